// The head of FTLMultiviewNet (lib/models/FTL_encoder_decoder.py): the feature transform layer and the 3x3 convolutions
// of its encoder and decoder, f32 NHWC.
//
// hrnet_ftl_gather / hrnet_ftl_scatter. The encoded map of a view is read as 3-vectors: per channel, triplets of
// consecutive pixels in row-major order (a triplet crosses a row boundary when the width is no multiple of 3). In NHWC
// the three members of a triplet sit one pixel row (ld floats) apart, so one thread takes a triplet x 4 channels: three
// 16-byte loads, 3 x 4 outputs  y_j = fma(x2, a[2][j], fma(x1, a[1][j], fma(x0, a[0][j], c[j])))  in that order, three
// 16-byte stores. The gather writes view v into channel slice v of the concatenated map (the concat is never a copy);
// the scatter reads the fused map ONCE and writes all V views, slot b V + v. No LDS, no atomics. Both move about 1 MB
// at full size (B x V = 1 x 4: 4 x 324 x 240 floats in, as much out): far below what fills the device's queues, so the
// grid is simply one thread per work item in 256-thread blocks - 102 of them there, one wave of blocks on 256 CUs, the
// launch itself is the cost - with a grid-stride loop capped at 8 blocks per CU for maps that are larger.
//
// hrnet_conv2d_3x3g: a 3x3 convolution with an explicit output size,
//   y[n,ho,wo,co] = relu?(bias[co] + sum_{r,s,ci} w[co][3 r + s][ci] xz[n, ho stride + r - pad_lo, wo stride + s - pad_lo, ci]),
//   xz[i] = x[i / z] when i % z == 0 and 0 <= i / z < H, else 0,
// as an implicit GEMM on the f32 MFMA (mfma_f32_16x16x4), on the LDS layout and MFMA order of conv_kxk_body.h. A
// workgroup owns 128 output pixels OF ONE PARITY CLASS (for z = 2: the outputs (2 a + ph, 2 b + pw) of one (ph, pw);
// for z = 1 there is one class) and a block of output channels: an 8 x 16 tile of the class's grid, or - where that needs
// fewer workgroups and the window fits, as for the head's 33 x 33 and 18 x 18 maps - a strip of 128 consecutive pixels of it
// in row-major order, whose window spans whole rows. For z = 2 the taps of a class that meet stuffed zeros
// are the same for all its outputs - (ph + r - pad_lo) odd or (pw + s - pad_lo) odd - and are skipped: 1, 2, 2 or 4 of
// the 9 taps are issued, and the window staged in LDS is one of REAL input pixels ((7 step + 3) x (15 step + 3) of them per
// 16 channels for an 8 x 16 tile, step = stride for z = 1 and 1 for z = 2), staged once for all taps. The weights ([Cout_pad][9][Cin] of
// hrnet_pack_weights) of the live taps of a 16-channel pass are requested from global memory before the window is
// staged, so their latency hides behind the staging.
//
// Summation order of one output (fixed: no atomics, no split K; the choice of tile variant changes which workgroup
// owns an output, not its sum, so B = 1 and B = 4 give equal bits):
//   acc = 0; for c0 = 0, 16, ... < Cin:
//       part = 0; for r = 0 .. 2; for s = 0 .. 2, live taps only; for j = 0 .. 3:
//           part = mfma_16x16x4(w[co][3 r + s][c0 + 4 g + j], x[.][c0 + 4 g + j], g = 0 .. 3, part)
//       acc += part
//   y = acc + bias; ReLU.
// A skipped tap would have added products with an exact zero: the sum is that of the dense form.
#include "conv_kxk_body.h"

namespace {

struct G3Args {
  const float* x;
  const float* w;
  const float* bias;
  float* y;
  int N, H, W, Cin, ldx, x_off, Cout, Cout_pad, ldy, y_off, Ho, Wo, stride, pad_lo, z, relu, tiles_h, tiles_w, vec_store;
  int Ha, Wa;   // outputs of a parity class per axis (the largest class): ceil(Ho / z), ceil(Wo / z)
};

// the 128 pixels of a tile are either KX_TH x KX_TW of the class's grid, or (LIN) 128 consecutive pixels of it in row-major
// order: rows of 33 or 18 outputs fill 8 x 16 tiles to 57 % and 42 %, strips of them to 95 % and 84 %. A strip's window
// spans whole rows; g3_strip_rows bounds how many (a strip starts anywhere in a row)
constexpr int G3_TILE = KX_TH * KX_TW, G3_STRIP_PIXELS = 768;   // the largest staged window of a strip: 48 KB of LDS
__host__ __device__ __forceinline__ int g3_strip_rows(int Wa) { return (G3_TILE - 1) / Wa + 2; }

// input step between neighbouring outputs of a class, and the input offset of the window's first row / column
__host__ __device__ __forceinline__ int g3_step(int z, int stride) { return z == 1 ? stride : 1; }
__host__ __device__ __forceinline__ int g3_base(int z, int pad_lo) { return z == 1 ? -pad_lo : -((pad_lo + 1) >> 1); }

template <int MT, int NT, int WM, int WN, bool LIN>
__global__ __launch_bounds__(256) void conv3x3g_kernel(const G3Args a) {
  static_assert(WM * WN == 4 && NT * WN == KX_TH, "tile");
  extern __shared__ V16 g3_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int wm = wave / WN, wn = wave % WN;
  const int z = a.z;
  int t = blockIdx.x;
  const int tw = t % a.tiles_w;
  t /= a.tiles_w;
  const int th = t % a.tiles_h;
  t /= a.tiles_h;
  const int cls = t % (z * z), n = t / (z * z);
  const int ph = cls / z, pw = cls % z;
  const int step = g3_step(z, a.stride), base = g3_base(z, a.pad_lo);
  // first output row / column of the tile, counted within its class, and the rows and columns of its input window
  int a0, b0, HH, WH;
  if constexpr (LIN) {
    const int last = min(tw * G3_TILE + G3_TILE - 1, a.Ha * a.Wa - 1);
    a0 = tw * G3_TILE / a.Wa;
    b0 = 0;
    HH = (last / a.Wa - a0) * step + 3;
    WH = (a.Wa - 1) * step + 3;
  } else {
    a0 = th * KX_TH;
    b0 = tw * KX_TW;
    HH = (KX_TH - 1) * step + 3;
    WH = (KX_TW - 1) * step + 3;
  }
  const int co_base = ((int)blockIdx.y * WM + wm) * MT * 16;
  const int row_base = wn * NT;
  const int Cin = a.Cin;
  const size_t wrow = (size_t)9 * Cin;
  const float* xn = a.x + (size_t)n * a.H * a.W * a.ldx + a.x_off;

  // which taps are live for this class, and where their input sits in the window (0 .. 2)
  bool rlive[3], clive[3];
  int roff[3], coff[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int dr = ph + r - a.pad_lo, dc = pw + r - a.pad_lo;
    rlive[r] = z == 1 || !(dr & 1);
    clive[r] = z == 1 || !(dc & 1);
    roff[r] = z == 1 ? r : (dr >> 1) - base;   // dr even where it is used: the shift is exact
    coff[r] = z == 1 ? r : (dc >> 1) - base;
  }

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

  // this lane's pixels: row and column within the class, and where their window starts in LDS. A pixel past the class
  // (the last strip) reads the window's first pixel and is never stored
  int pa[NT], pb[NT], pix[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    if constexpr (LIN) {
      const int p = tw * G3_TILE + (row_base + q) * KX_TW + li;
      const bool ok = p < a.Ha * a.Wa;
      pa[q] = ok ? p / a.Wa : a.Ha;
      pb[q] = ok ? p - pa[q] * a.Wa : 0;
      pix[q] = ok ? (pa[q] - a0) * step * WH + pb[q] * step : 0;
    } else {
      pa[q] = a0 + row_base + q;
      pb[q] = b0 + li;
      pix[q] = (row_base + q) * step * WH + li * step;
    }
  }
  const int h_first = a0 * step + base, w_first = b0 * step + base;
  for (int c0 = 0; c0 < Cin; c0 += KX_KC) {
    const int c = c0 + lg * 4;
    const bool cok = c < Cin;   // a pass past Cin: zero weights against the zero vectors staged below
    V16 wr[9][MT];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int m = 0; m < MT; ++m)
          wr[3 * r + s][m] = rlive[r] && clive[s] && cok && wok[m] ? *(const V16*)(wl[m] + (size_t)(3 * r + s) * Cin + c)
                                                                    : v16_zero();
    __syncthreads();   // the taps of the previous pass have read the window
    for (int v = tid; v < HH * WH * 4; v += 256) {
      const int p = v >> 2, g = v & 3;
      const int hr = p / WH, wc = p - hr * WH;
      const int h = h_first + hr, w = w_first + wc, cc = c0 + g * 4;
      V16 val = v16_zero();
      if (h >= 0 && h < a.H && w >= 0 && w < a.W && cc < Cin) val = *(const V16*)(xn + ((size_t)h * a.W + w) * a.ldx + cc);
      g3_lds[kx_slot(p, g)] = val;
    }
    __syncthreads();
    f32x4 part[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int q = 0; q < NT; ++q) part[m][q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      if (!rlive[r]) continue;   // uniform over the workgroup
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        if (!clive[s]) continue;
        V16 bv[NT];
#pragma unroll
        for (int q = 0; q < NT; ++q)
          bv[q] = g3_lds[kx_slot(pix[q] + roff[r] * WH + coff[s], lg)];
        kx_mma<MT, NT>(wr[3 * r + s], bv, part);
      }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int q = 0; q < NT; ++q) acc[m][q] += part[m][q];
  }

  // D of the 16x16 MFMA: column (pixel) = lane & 15, row (output channel) = 4 (lane >> 4) + register
  float* yn = a.y + (size_t)n * a.Ho * a.Wo * a.ldy + a.y_off;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int ho = pa[q] * z + ph, wo = pb[q] * z + pw;
    if (ho >= a.Ho || wo >= a.Wo) continue;
    float* yp = yn + ((size_t)ho * a.Wo + wo) * a.ldy;
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

// pixels of the window a strip may stage
long long g3_strip_window(int Wa, int step) {
  return (long long)((g3_strip_rows(Wa) - 1) * step + 3) * ((long long)(Wa - 1) * step + 3);
}

template <int MT, int NT, int WM, int WN>
void g3_launch(const G3Args& a, bool lin, hipStream_t s) {
  const int step = g3_step(a.z, a.stride);
  const int cb = 16 * MT * WM;
  const dim3 grid((unsigned)(a.N * a.z * a.z * a.tiles_h * a.tiles_w), (unsigned)((a.Cout_pad + cb - 1) / cb));
  if (lin)
    hipLaunchKernelGGL((conv3x3g_kernel<MT, NT, WM, WN, true>), grid, dim3(256), (size_t)g3_strip_window(a.Wa, step) * 64, s, a);
  else
    hipLaunchKernelGGL((conv3x3g_kernel<MT, NT, WM, WN, false>), grid, dim3(256),
                       (size_t)((KX_TH - 1) * step + 3) * ((KX_TW - 1) * step + 3) * 64, s, a);
}

// y (B, P, ldy) slice v <- x (B V, P, ldx) A_bv + c_bv, per triplet of pixels and channel
__global__ __launch_bounds__(256) void ftl_gather_kernel(const float* __restrict__ x, const float* __restrict__ coef,
                                                         float* __restrict__ y, int B, int V, int T, int C4, int ldx,
                                                         int x_off, int ldy, int y_off, int slice) {
  const long long total = (long long)B * V * T * C4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int cg = (int)(i % C4);
    long long q = i / C4;
    const int tr = (int)(q % T);
    const int bv = (int)(q / T), b = bv / V, v = bv - b * V;
    const float* k = coef + (size_t)bv * 12;
    const float* xp = x + ((size_t)bv * T * 3 + (size_t)tr * 3) * ldx + x_off + cg * 4;
    const f32x4 x0 = *(const f32x4*)xp, x1 = *(const f32x4*)(xp + ldx), x2 = *(const f32x4*)(xp + 2 * (size_t)ldx);
    float* yp = y + ((size_t)b * T * 3 + (size_t)tr * 3) * ldy + y_off + (size_t)v * slice + cg * 4;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = fmaf(x2[e], k[6 + j], fmaf(x1[e], k[3 + j], fmaf(x0[e], k[j], k[9 + j])));
      *(f32x4*)(yp + (size_t)j * ldy) = o;
    }
  }
}

// y (B V, P, ldy) slot b V + v <- f (B, P, ldf) A_bv + c_bv for all V views from one read of f
__global__ __launch_bounds__(256) void ftl_scatter_kernel(const float* __restrict__ f, const float* __restrict__ coef,
                                                          float* __restrict__ y, int B, int V, int T, int C4, int ldf,
                                                          int f_off, int ldy, int y_off) {
  const long long total = (long long)B * T * C4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int cg = (int)(i % C4);
    long long q = i / C4;
    const int tr = (int)(q % T), b = (int)(q / T);
    const float* fp = f + ((size_t)b * T * 3 + (size_t)tr * 3) * ldf + f_off + cg * 4;
    const f32x4 x0 = *(const f32x4*)fp, x1 = *(const f32x4*)(fp + ldf), x2 = *(const f32x4*)(fp + 2 * (size_t)ldf);
    for (int v = 0; v < V; ++v) {
      const int bv = b * V + v;
      const float* k = coef + (size_t)bv * 12;
      float* yp = y + ((size_t)bv * T * 3 + (size_t)tr * 3) * ldy + y_off + cg * 4;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaf(x2[e], k[6 + j], fmaf(x1[e], k[3 + j], fmaf(x0[e], k[j], k[9 + j])));
        *(f32x4*)(yp + (size_t)j * ldy) = o;
      }
    }
  }
}

unsigned ftl_grid(long long total) {
  const long long b = (total + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

int ftl_check(const char* who, const void* src, const void* coef, const void* dst, int B, int V, int H, int W, int C,
              int ld_in, int in_off, int ld_out, int out_off, long long out_width) {
  HR_REQUIRE(src && coef && dst, "%s: null argument", who);
  HR_REQUIRE(B >= 1 && V >= 1 && H >= 1 && W >= 1 && C >= 1, "%s: B = %d, V = %d, H = %d, W = %d, C = %d", who, B, V, H, W,
             C);
  HR_REQUIRE((long long)B * V <= 0x7fffffffLL && (long long)H * W <= 0x7fffffffLL, "%s: B V = %lld, H W = %lld", who,
             (long long)B * V, (long long)H * W);
  HR_REQUIRE(((long long)H * W) % 3 == 0, "%s: H W = %d x %d = %lld pixels are no whole number of triplets", who, H, W,
             (long long)H * W);
  HR_REQUIRE(C % 4 == 0 && ld_in % 4 == 0 && in_off % 4 == 0 && ld_out % 4 == 0 && out_off % 4 == 0,
             "%s: C = %d, ld = %d / %d, offsets %d / %d: multiples of 4", who, C, ld_in, ld_out, in_off, out_off);
  HR_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0 && ((uintptr_t)coef & 3) == 0,
             "%s: the maps must be 16-byte aligned", who);
  HR_REQUIRE(in_off >= 0 && (long long)in_off + C <= ld_in, "%s: input channels [%d, %d + %d) outside ld = %d", who, in_off,
             in_off, C, ld_in);
  HR_REQUIRE(out_off >= 0 && (long long)out_off + out_width <= ld_out,
             "%s: output channels [%d, %d + %lld) outside ld = %d", who, out_off, out_off, out_width, ld_out);
  return HR_OK;
}

}  // namespace

extern "C" int hrnet_ftl_gather(const float* x, const float* coef, float* y, int B, int V, int H, int W, int C, int ldx,
                                int x_off, int ldy, int y_off, int slice, hr_stream_t stream) {
  HR_REQUIRE(slice >= C && slice % 4 == 0, "ftl_gather: slice = %d: a multiple of 4 that holds C = %d", slice, C);
  const int rc = ftl_check("ftl_gather", x, coef, y, B, V, H, W, C, ldx, x_off, ldy, y_off,
                           (long long)(V - 1) * slice + C);
  if (rc != HR_OK) return rc;
  const int T = (int)((long long)H * W / 3);
  hipLaunchKernelGGL(ftl_gather_kernel, dim3(ftl_grid((long long)B * V * T * (C / 4))), dim3(256), 0, (hipStream_t)stream, x,
                     coef, y, B, V, T, C / 4, ldx, x_off, ldy, y_off, slice);
  return hr_check_launch("ftl_gather");
}

extern "C" int hrnet_ftl_scatter(const float* f, const float* coef, float* y, int B, int V, int H, int W, int C, int ldf,
                                 int f_off, int ldy, int y_off, hr_stream_t stream) {
  const int rc = ftl_check("ftl_scatter", f, coef, y, B, V, H, W, C, ldf, f_off, ldy, y_off, C);
  if (rc != HR_OK) return rc;
  const int T = (int)((long long)H * W / 3);
  hipLaunchKernelGGL(ftl_scatter_kernel, dim3(ftl_grid((long long)B * T * (C / 4))), dim3(256), 0, (hipStream_t)stream, f,
                     coef, y, B, V, T, C / 4, ldf, f_off, ldy, y_off);
  return hr_check_launch("ftl_scatter");
}

extern "C" int hrnet_conv2d_3x3g(int dtype, const void* x, const void* w, const float* bias, void* y, int N, int H, int W,
                                 int Cin, int ldx, int x_off, int Cout, int ldy, int y_off, int Ho, int Wo, int stride,
                                 int pad_lo, int z, int relu, hr_stream_t stream) {
  HR_REQUIRE(dtype == HR_F32, "conv2d_3x3g: dtype = %d: only f32 (HR_F32 = 0) is built", dtype);
  HR_REQUIRE(x && w && y, "conv2d_3x3g: null argument");
  HR_REQUIRE(N >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1 && H <= 0x3fffffff && W <= 0x3fffffff,
             "conv2d_3x3g: N = %d, H = %d, W = %d, Cin = %d, Cout = %d", N, H, W, Cin, Cout);
  HR_REQUIRE((stride == 1 || stride == 2) && pad_lo >= 0 && pad_lo <= 2 && (z == 1 || (z == 2 && stride == 1)),
             "conv2d_3x3g: stride = %d (1, 2), pad_lo = %d (0 .. 2), z = %d (1, or 2 with stride 1)", stride, pad_lo, z);
  // an output size between that of no padding behind the map and that of two rows / columns of it: no output depends
  // on padding alone beyond them
  {
    const long long Hz = (long long)(H - 1) * z + 1, Wz = (long long)(W - 1) * z + 1;
    const long long hlo = Hz + pad_lo - 3 < 0 ? 1 : (Hz + pad_lo - 3) / stride + 1, hhi = (Hz + pad_lo - 1) / stride + 1;
    const long long wlo = Wz + pad_lo - 3 < 0 ? 1 : (Wz + pad_lo - 3) / stride + 1, whi = (Wz + pad_lo - 1) / stride + 1;
    HR_REQUIRE(Ho >= hlo && Ho <= hhi && Wo >= wlo && Wo <= whi,
               "conv2d_3x3g: Ho x Wo = %d x %d: H = %d, W = %d, z = %d, stride = %d, pad_lo = %d give %lld .. %lld x %lld .. %lld",
               Ho, Wo, H, W, z, stride, pad_lo, hlo, hhi, wlo, whi);
  }
  HR_REQUIRE(Cin % 4 == 0 && ldx % 4 == 0 && x_off % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0,
             "conv2d_3x3g: Cin = %d, ldx = %d, x_off = %d: multiples of 4, x and w 16-byte aligned", Cin, ldx, x_off);
  HR_REQUIRE(x_off >= 0 && (long long)x_off + Cin <= ldx, "conv2d_3x3g: channels [%d, %d + %d) outside ldx = %d", x_off,
             x_off, Cin, ldx);
  HR_REQUIRE(y_off >= 0 && (long long)y_off + Cout <= ldy, "conv2d_3x3g: channels [%d, %d + %d) outside ldy = %d", y_off,
             y_off, Cout, ldy);
  HR_REQUIRE(((uintptr_t)y & 3) == 0 && (relu == 0 || relu == 1), "conv2d_3x3g: y alignment / relu = %d", relu);
  HR_REQUIRE(Cout <= 0x7fffffff - 15, "conv2d_3x3g: Cout = %d", Cout);
  G3Args a;
  a.x = (const float*)x; a.w = (const float*)w; a.bias = bias; a.y = (float*)y;
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ldx = ldx; a.x_off = x_off; a.Cout = Cout; a.Cout_pad = (Cout + 15) / 16 * 16;
  a.ldy = ldy; a.y_off = y_off; a.Ho = Ho; a.Wo = Wo; a.stride = stride; a.pad_lo = pad_lo; a.z = z; a.relu = relu;
  a.vec_store = ldy % 4 == 0 && y_off % 4 == 0 && ((uintptr_t)y & 15) == 0;
  a.Ha = (Ho + z - 1) / z;
  a.Wa = (Wo + z - 1) / z;
  a.tiles_h = (a.Ha + KX_TH - 1) / KX_TH;
  a.tiles_w = (a.Wa + KX_TW - 1) / KX_TW;
  // strips where they need fewer tiles than the 8 x 16 grid and their window fits: a function of the output size and the
  // geometry alone, and the sums are the same either way
  const long long strips = ((long long)a.Ha * a.Wa + G3_TILE - 1) / G3_TILE;
  const bool lin = strips < (long long)a.tiles_h * a.tiles_w &&
                   g3_strip_window(a.Wa, g3_step(z, stride)) <= G3_STRIP_PIXELS;
  if (lin) {
    a.tiles_h = 1;
    a.tiles_w = (int)strips;
  }
  const long long ptiles = (long long)N * z * z * a.tiles_h * a.tiles_w;
  HR_REQUIRE(ptiles <= 0x7fffffffLL, "conv2d_3x3g: %lld pixel tiles", ptiles);
  // the tile variants of hrnet_conv2d_kxk, by the same rule (conv_kxk_body.h): the sums do not depend on the choice
  if (a.Cout_pad % 64 == 0 && ptiles * (a.Cout_pad / 64) >= 512)
    g3_launch<1, 8, 4, 1>(a, lin, (hipStream_t)stream);
  else if (ptiles * ((a.Cout_pad + 31) / 32) >= 256)
    g3_launch<1, 4, 2, 2>(a, lin, (hipStream_t)stream);
  else
    g3_launch<1, 2, 1, 4>(a, lin, (hipStream_t)stream);
  return hr_check_launch("conv2d_3x3g");
}
