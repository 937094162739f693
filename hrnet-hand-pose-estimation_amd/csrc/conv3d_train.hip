// V2V training (reference lib/models/v2v.py in train mode): what csrc/conv3d.hip lacks for a training step. f32 only,
// NDHWC with 64-bit offsets, no atomics anywhere: every sum has one fixed order, so a call is bit-reproducible.
//
//   BatchNorm3d over rows = N*D*H*W   two passes over the raw convolution output z: per-workgroup partial sums of z, then
//                                     of (z - mean)^2 around the mean those partials give (never E[z^2] - E[z]^2), then
//                                     one finalising launch. A thread sums its rows in f32, the row lanes of a workgroup
//                                     are added through LDS in lane order, the workgroups in index order in f64.
//   BatchNorm backward                the same partial scheme for sum g and sum g * xhat, g = dy masked by the ReLU; the
//                                     apply kernel writes dz and, for a residual input, g itself.
//   weight gradient                   dW[tap][co][ci] = sum_v dz[v,co] x[v+tap,ci] as a GEMM whose K is the voxel count:
//                                     mfma_f32_16x16x4f32 with A = dz (row = co, k = voxel), B = x (k = voxel, col = ci).
//                                     A wave owns one tap, 16 * MB output and 16 * NBI input channels and one split of
//                                     the voxels; a second kernel adds the splits in index order into OIDHW (or IODHW).
//   max-pool backward                 the argmax is recomputed from the saved input: first maximum in (d, h, w) order.
//   deconvolution k2s2 backward       input gradient: the conv body with the fine voxel 2v + tap LOADED per tap
//                                     (K = 8 * Cout); weight gradient: the kernel above with the stride-2 voxel map.
// The input gradient of Conv3d is hrnet_conv3d itself on dz with the weights of hrnet_pack_weights3d_dgrad.
#include "common.h"

namespace {

constexpr long long kMaxVox = 1LL << 36;
constexpr int kBnThreads = 256;
constexpr int kBnMaxParts = 256;      // partial rows of the BatchNorm sums (one per workgroup)
constexpr int kBnMaxC = 1024;         // C / 4 channel quads fit one workgroup
constexpr int kSplitVox = 2048;       // voxels of one weight-gradient split, until kMaxSplits of them are in use
constexpr int kMaxSplits = 256;

int t3_channels_ok(int Cin, int Cout) {
  return Cin >= 4 && Cin % 4 == 0 && Cout >= 16 && Cout % 16 == 0 && Cin <= 4096 && Cout <= 4096;
}

// a * b * c * d of positive ints, or kMaxVox + 1 once it passes kMaxVox (the plain product overflows 64 bits)
long long t3_product(int a, int b, int c, int d) {
  long long r = a;
  for (const int f : {b, c, d}) {
    r *= f;
    if (r > kMaxVox) return kMaxVox + 1;
  }
  return r;
}

int t3_rows(const char* what, int dtype, int N, int D, int H, int W, long long* rows) {
  HR_REQUIRE(dtype == HR_F32, "%s: dtype = %d: only f32 (HR_F32 = 0) is built", what, dtype);
  HR_REQUIRE(N >= 1 && D >= 1 && H >= 1 && W >= 1, "%s: N = %d, D = %d, H = %d, W = %d", what, N, D, H, W);
  *rows = t3_product(N, D, H, W);
  HR_REQUIRE(*rows <= kMaxVox, "%s: N * D * H * W = more than 2^36 voxels (N = %d, D = %d, H = %d, W = %d)", what, N, D,
             H, W);
  return HR_OK;
}

int bn_parts(long long rows) {
  const long long p = (rows + 255) / 256;
  return (int)(p < 1 ? 1 : (p > kBnMaxParts ? kBnMaxParts : p));
}

// ---------------------------------------------------------------------------------------------------------------------
// BatchNorm sums. Thread t of a workgroup: channel quad q = t % (C / 4), row lane r = t / (C / 4) of RL = 256 / (C / 4);
// workgroup b owns rows [b * per, (b + 1) * per). MODE 0: sum z. MODE 1: sum (z - mean)^2, the mean from the MODE 0
// partials. MODE 2: sum g and sum g * xhat (backward).
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 bn_mean_of(const float* __restrict__ part, int nparts, int C, int c, double rows) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = 0; p < nparts; ++p) {
    const f32x4 v = *(const f32x4*)(part + (long long)p * C + c);
    s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
  }
  return f32x4{(float)(s[0] / rows), (float)(s[1] / rows), (float)(s[2] / rows), (float)(s[3] / rows)};
}

__device__ __forceinline__ f32x4 bn_lanes_sum(f32x4 v, f32x4* lds, int q, int r, int quads, int RL) {
  __syncthreads();
  if (r < RL) lds[r * quads + q] = v;
  __syncthreads();
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (r == 0)
    for (int k = 0; k < RL; ++k) s += lds[k * quads + q];
  return s;
}

// g = dy where the ReLU let the forward through. mask_y: the saved output (y > 0); or, where something was added after
// the ReLU, recomputed as fmaf(z, scale, shift) > 0 - the forward's own expression, so the same bits decide.
__device__ __forceinline__ f32x4 bn_masked(f32x4 g, const float* mask_y, const float* scale, const float* shift,
                                           f32x4 z, long long at, int c) {
  if (mask_y) {
    const f32x4 y = *(const f32x4*)(mask_y + at);
    g.x = y.x > 0.f ? g.x : 0.f; g.y = y.y > 0.f ? g.y : 0.f; g.z = y.z > 0.f ? g.z : 0.f; g.w = y.w > 0.f ? g.w : 0.f;
  } else if (scale) {
    const f32x4 sc = *(const f32x4*)(scale + c), sh = *(const f32x4*)(shift + c);
    g.x = fmaf(z.x, sc.x, sh.x) > 0.f ? g.x : 0.f; g.y = fmaf(z.y, sc.y, sh.y) > 0.f ? g.y : 0.f;
    g.z = fmaf(z.z, sc.z, sh.z) > 0.f ? g.z : 0.f; g.w = fmaf(z.w, sc.w, sh.w) > 0.f ? g.w : 0.f;
  }
  return g;
}

template <int MODE>
__global__ __launch_bounds__(kBnThreads) void bn3d_sums_kernel(const float* __restrict__ z, const float* __restrict__ dy,
                                                               const float* __restrict__ mask_y,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ shift,
                                                               const float* __restrict__ mean_in,
                                                               const float* __restrict__ invstd_in,
                                                               const float* __restrict__ part_in, float* __restrict__ out0,
                                                               float* __restrict__ out1, long long rows, int C,
                                                               long long per, int nparts) {
  __shared__ f32x4 lds[kBnThreads];
  const int quads = C >> 2, RL = kBnThreads / quads;
  const int q = threadIdx.x % quads, r = threadIdx.x / quads, c = q * 4;
  const long long r0 = (long long)blockIdx.x * per;
  const long long r1 = r0 + per < rows ? r0 + per : rows;
  f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, b = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 mean = f32x4{0.f, 0.f, 0.f, 0.f}, istd = f32x4{0.f, 0.f, 0.f, 0.f};
  if (MODE == 1) mean = bn_mean_of(part_in, nparts, C, c, (double)rows);
  if (MODE == 2 && z) { mean = *(const f32x4*)(mean_in + c); istd = *(const f32x4*)(invstd_in + c); }
  if (r < RL)
    for (long long row = r0 + r; row < r1; row += RL) {
      const long long at = row * C + c;
      if (MODE == 0) {
        a += *(const f32x4*)(z + at);
      } else if (MODE == 1) {
        const f32x4 d = *(const f32x4*)(z + at) - mean;
        a.x = fmaf(d.x, d.x, a.x); a.y = fmaf(d.y, d.y, a.y); a.z = fmaf(d.z, d.z, a.z); a.w = fmaf(d.w, d.w, a.w);
      } else {
        const f32x4 zz = z ? *(const f32x4*)(z + at) : f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 g = bn_masked(*(const f32x4*)(dy + at), mask_y, scale, shift, zz, at, c);
        const f32x4 xh = (zz - mean) * istd;
        a += g;
        b.x = fmaf(g.x, xh.x, b.x); b.y = fmaf(g.y, xh.y, b.y); b.z = fmaf(g.z, xh.z, b.z); b.w = fmaf(g.w, xh.w, b.w);
      }
    }
  a = bn_lanes_sum(a, lds, q, r, quads, RL);
  if (MODE == 2) b = bn_lanes_sum(b, lds, q, r, quads, RL);
  if (r == 0) {
    *(f32x4*)(out0 + (long long)blockIdx.x * C + c) = a;
    if (MODE == 2) *(f32x4*)(out1 + (long long)blockIdx.x * C + c) = b;
  }
}

// one thread per channel: the partials in index order in f64; writes mean, invstd, scale, shift and the running statistics
__global__ __launch_bounds__(64) void bn3d_finalize_kernel(const float* __restrict__ psum, const float* __restrict__ psq,
                                                           int nparts, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ mean,
                                                           float* __restrict__ invstd, float* __restrict__ scale,
                                                           float* __restrict__ shift, float* __restrict__ running_mean,
                                                           float* __restrict__ running_var,
                                                           long long* __restrict__ num_batches_tracked, double rows,
                                                           float momentum, float eps, int C, int Creal) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c == 0 && num_batches_tracked) *num_batches_tracked += 1;
  if (c >= C) return;
  double s = 0.0, sq = 0.0;
  for (int p = 0; p < nparts; ++p) { s += psum[(long long)p * C + c]; sq += psq[(long long)p * C + c]; }
  const float m = (float)(s / rows);              // the mean the second pass centred on: the same expression
  const double var = sq / rows;
  const float is = (float)(1.0 / sqrt(var + (double)eps));
  const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
  const float sc = g * is;
  mean[c] = m;
  invstd[c] = is;
  scale[c] = sc;
  shift[c] = fmaf(-m, sc, bt);
  if (c < Creal && running_mean) {
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)(var * (rows / (rows - 1.0)));
  }
}

// y = z * scale + shift; after_relu == 0: + other, ReLU (Res3DBlock); after_relu != 0: ReLU, + other (the decoder)
__global__ __launch_bounds__(256) void bn3d_apply_kernel(const float* __restrict__ z, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, const float* __restrict__ other,
                                                         float* __restrict__ y, long long total, int C, int relu,
                                                         int after_relu) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % (C >> 2)) * 4;
  const f32x4 sc = *(const f32x4*)(scale + c), sh = *(const f32x4*)(shift + c);
  f32x4 v = *(const f32x4*)(z + i * 4);
  v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y); v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
  if (other && !after_relu) v += *(const f32x4*)(other + i * 4);
  if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
  if (other && after_relu) v += *(const f32x4*)(other + i * 4);
  *(f32x4*)(y + i * 4) = v;
}

// one thread per channel. With a BatchNorm (has_bn): coef[c] = sum g / rows, coef[C + c] = sum g xhat / rows,
// dgamma = sum g xhat, dbeta = sum g, and the convolution's bias gradient sum dz = scale * (sum g - rows * mean g -
// mean(g xhat) * sum xhat): the first two cancel and sum xhat is zero by the definition of the batch mean, so it is
// written as the zero it is. Without one (the output layer): dbias = sum g.
__global__ __launch_bounds__(64) void bn3d_bwd_finalize_kernel(const float* __restrict__ pg, const float* __restrict__ pgx,
                                                               int nparts, double rows, float* __restrict__ coef,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                               float* __restrict__ dbias, int C, int Creal, int has_bn,
                                                               int accumulate) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, sx = 0.0;
  for (int p = 0; p < nparts; ++p) { s += pg[(long long)p * C + c]; sx += pgx[(long long)p * C + c]; }
  if (coef) { coef[c] = (float)(s / rows); coef[C + c] = (float)(sx / rows); }
  if (c >= Creal) return;
  if (has_bn) {
    if (dgamma) dgamma[c] = (accumulate ? dgamma[c] : 0.f) + (float)sx;
    if (dbeta) dbeta[c] = (accumulate ? dbeta[c] : 0.f) + (float)s;
    if (dbias && !accumulate) dbias[c] = 0.f;
  } else if (dbias) {
    dbias[c] = (accumulate ? dbias[c] : 0.f) + (float)s;
  }
}

// dz = scale * (g - mean g - xhat * mean(g xhat)); dother (+)= g for a residual input
__global__ __launch_bounds__(256) void bn3d_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ z,
                                                             const float* __restrict__ mask_y,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ invstd,
                                                             const float* __restrict__ coef, float* __restrict__ dz,
                                                             float* __restrict__ dother, long long total, int C,
                                                             int recompute, int accumulate_other) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % (C >> 2)) * 4;
  const f32x4 zz = *(const f32x4*)(z + i * 4);
  const f32x4 g = bn_masked(*(const f32x4*)(dy + i * 4), mask_y, recompute ? scale : nullptr, shift, zz, i * 4, c);
  const f32x4 xh = (zz - *(const f32x4*)(mean + c)) * *(const f32x4*)(invstd + c);
  const f32x4 mg = *(const f32x4*)(coef + c), mgx = *(const f32x4*)(coef + C + c), sc = *(const f32x4*)(scale + c);
  f32x4 v;
  v.x = sc.x * (g.x - mg.x - xh.x * mgx.x); v.y = sc.y * (g.y - mg.y - xh.y * mgx.y);
  v.z = sc.z * (g.z - mg.z - xh.z * mgx.z); v.w = sc.w * (g.w - mg.w - xh.w * mgx.w);
  *(f32x4*)(dz + i * 4) = v;
  if (dother) {
    f32x4 o = g;
    if (accumulate_other) o += *(const f32x4*)(dother + i * 4);
    *(f32x4*)(dother + i * 4) = o;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// max-pool backward: one thread per OUTPUT voxel and 4 channels writes all 8 inputs of its window (every input voxel
// lies in exactly one window: nothing is zeroed beforehand, nothing is added from two threads)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool3d_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                            float* __restrict__ dx, long long total, int Do, int Ho,
                                                            int Wo, int C, int accumulate) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c4 = C >> 2;
  const int c = (int)(i % c4) * 4;
  long long q = i / c4;
  const int w = (int)(q % Wo); q /= Wo;
  const int h = (int)(q % Ho); q /= Ho;
  const int d = (int)(q % Do);
  const long long n = q / Do;
  const int H = 2 * Ho, W = 2 * Wo;
  const long long first = (((n * (2 * Do) + 2 * d) * H + 2 * h) * (long long)W + 2 * w) * C + c;
  f32x4 m = *(const f32x4*)(x + first);
  int ax = 0, ay = 0, az = 0, aw = 0;
#pragma unroll
  for (int t = 1; t < 8; ++t) {
    const long long at = first + (((long long)(t >> 2) * H + ((t >> 1) & 1)) * W + (t & 1)) * C;
    const f32x4 v = *(const f32x4*)(x + at);
    if (v.x > m.x) { m.x = v.x; ax = t; }          // strict: the first maximum in (d, h, w) order keeps it
    if (v.y > m.y) { m.y = v.y; ay = t; }
    if (v.z > m.z) { m.z = v.z; az = t; }
    if (v.w > m.w) { m.w = v.w; aw = t; }
  }
  const f32x4 g = *(const f32x4*)(dy + i * 4);
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const long long at = first + (((long long)(t >> 2) * H + ((t >> 1) & 1)) * W + (t & 1)) * C;
    f32x4 o = f32x4{ax == t ? g.x : 0.f, ay == t ? g.y : 0.f, az == t ? g.z : 0.f, aw == t ? g.w : 0.f};
    if (accumulate) o += *(const f32x4*)(dx + at);
    *(f32x4*)(dx + at) = o;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// weights for the input gradient of Conv3d: out[tap][ci][co] = w[co][ci][taps - 1 - tap] (transposed and tap-reversed),
// ci < Cin_pad (a multiple of 16: it is the output side now), co < Cout_pad, zero beyond the real counts
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_weights3d_dgrad_kernel(const float* __restrict__ w, float* __restrict__ out,
                                                                   int Cout, int Cin, int taps, int Cout_pad,
                                                                   int Cin_pad, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int co = (int)(i % Cout_pad), ci = (int)((i / Cout_pad) % Cin_pad), t = (int)(i / ((long long)Cin_pad * Cout_pad));
  out[i] = (ci < Cin && co < Cout) ? w[((long long)co * Cin + ci) * taps + (taps - 1 - t)] : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------
// deconvolution k2s2, input gradient: dx[v,ci] = sum over the 8 taps and co of w[tap][ci][co] * dz[fine(v, tap), co].
// The body of conv3d_kernel with the tap's voxel LOADED from the fine volume; wp is [8][Cin][Cout] (pack_weights3d of
// the IODHW weight with the roles of the two channel counts exchanged).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kMP = 4, kWaves = 4, kWaveVox = 16 * kMP, kBlockVox = kWaveVox * kWaves;

__device__ __forceinline__ f32x4 mma4(const f32x4& a, const f32x4& b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
  return c;
}

template <int NB>
__global__ __launch_bounds__(64 * kWaves) void deconv3d_dgrad_kernel(const float* __restrict__ dz,
                                                                     const float* __restrict__ wp, float* __restrict__ dx,
                                                                     long long nvox, int D, int H, int W, int Cin,
                                                                     int Cout, int accumulate) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int cb = blockIdx.y * (16 * NB);           // block of INPUT channels (the rows of this product)
  const long long base = (long long)blockIdx.x * kBlockVox + (long long)wave * kWaveVox;
  if (base >= nvox) return;                        // the whole wave

  long long p[kMP], fine[kMP];
#pragma unroll
  for (int m = 0; m < kMP; ++m) {
    p[m] = base + m * 16 + j;
    const long long q = p[m] < nvox ? p[m] : nvox - 1;
    const int pw = (int)(q % W), ph = (int)((q / W) % H), pd = (int)((q / ((long long)W * H)) % D);
    const long long n = q / ((long long)W * H * D);
    fine[m] = ((n * (2 * D) + 2 * pd) * (2 * H) + 2 * ph) * (2LL * W) + 2 * pw;
  }
  f32x4 acc[kMP][NB];
#pragma unroll
  for (int m = 0; m < kMP; ++m)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[m][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int t = 0; t < 8; ++t) {
    const long long tshift = ((long long)(t >> 2) * (2 * H) + ((t >> 1) & 1)) * (2LL * W) + (t & 1);
    const float* wt = wp + ((long long)t * Cin + cb + j) * Cout + g * 4;
    for (int c0 = 0; c0 < Cout; c0 += 16) {
      f32x4 a[NB], b[kMP];
#pragma unroll
      for (int n = 0; n < NB; ++n) a[n] = *(const f32x4*)(wt + (long long)n * 16 * Cout + c0);
#pragma unroll
      for (int m = 0; m < kMP; ++m)
        b[m] = p[m] < nvox ? *(const f32x4*)(dz + (fine[m] + tshift) * Cout + c0 + g * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int m = 0; m < kMP; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[m][n] = mma4(a[n], b[m], acc[m][n]);
    }
  }
#pragma unroll
  for (int m = 0; m < kMP; ++m) {
    if (p[m] >= nvox) continue;
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      float* o = dx + p[m] * Cin + cb + n * 16 + 4 * g;
      f32x4 v = acc[m][n];
      if (accumulate) v += *(const f32x4*)o;
      *(f32x4*)o = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// weight gradient. grid = (splits, taps, co blocks * ci blocks), one wave per workgroup. The wave walks its split's
// voxels 16 at a time: lane (j, g) holds, for i = 0..3, voxel v = v0 + 4 i + g - its dz[v, co0 + 16 m + j] and its
// x[xv, ci0 + 16 n + j], xv = v + tap shift (zero outside the volume) or, DECONV, x at the coarse voxel v with dz at the
// fine voxel 2 v + tap. The (d, h, w, n) of a lane's voxel advance by 4 per step with carries, no division in the loop.
// part[split][tap][co][ci], ci < Cin16 (Cin rounded up to 16; the columns past Cin hold zeros).
// ---------------------------------------------------------------------------------------------------------------------
template <int MB, int NBI, bool DECONV>
__global__ __launch_bounds__(64) void conv3d_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                          float* __restrict__ part, long long nvox, long long per, int D,
                                                          int H, int W, int Cin, int Cout, int Cin16, int ks,
                                                          int ci_blocks) {
  const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
  const int t = blockIdx.y, taps = gridDim.y;
  const int co0 = (blockIdx.z / ci_blocks) * (16 * MB), ci0 = (blockIdx.z % ci_blocks) * (16 * NBI);
  const long long v0 = (long long)blockIdx.x * per;
  const long long v1 = v0 + per < nvox ? v0 + per : nvox;
  int dd = 0, dh = 0, dw = 0;
  if (DECONV) {
    dd = t >> 2; dh = (t >> 1) & 1; dw = t & 1;
  } else {
    const int half = ks >> 1;
    dw = t % ks - half; dh = (t / ks) % ks - half; dd = t / (ks * ks) - half;
  }
  // the lane's first voxel; every later one is 4 further
  long long v = v0 + g;
  const long long q = v < nvox ? v : 0;              // coordinates of a voxel past the end are never used: v < v1 gates
  int pw = (int)(q % W), ph = (int)((q / W) % H), pd = (int)((q / ((long long)W * H)) % D);
  long long pn = q / ((long long)W * H * D);

  f32x4 acc[MB][NBI];
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int n = 0; n < NBI; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  bool colok[NBI];
#pragma unroll
  for (int n = 0; n < NBI; ++n) colok[n] = ci0 + 16 * n + j < Cin;

  for (long long it = v0; it < v1; it += 16) {       // wave-uniform trip count
    float a[4][MB], b[4][NBI];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bool ok = v < v1;
      long long xv, zv;
      if (DECONV) {
        xv = v;
        zv = ((pn * (2 * D) + 2 * pd + dd) * (2 * H) + 2 * ph + dh) * (2LL * W) + 2 * pw + dw;
      } else {
        zv = v;
        xv = v + ((long long)dd * H + dh) * W + dw;
        ok = ok && (unsigned)(pd + dd) < (unsigned)D && (unsigned)(ph + dh) < (unsigned)H &&
             (unsigned)(pw + dw) < (unsigned)W;
      }
#pragma unroll
      for (int m = 0; m < MB; ++m) a[i][m] = ok ? dz[zv * Cout + co0 + 16 * m + j] : 0.f;
#pragma unroll
      for (int n = 0; n < NBI; ++n) b[i][n] = (ok && colok[n]) ? x[xv * Cin + ci0 + 16 * n + j] : 0.f;
      v += 4;
      pw += 4;
      while (pw >= W) {
        pw -= W;
        if (++ph >= H) {
          ph = 0;
          if (++pd >= D) { pd = 0; ++pn; }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int n = 0; n < NBI; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][m], b[i][n], acc[m][n], 0, 0, 0);
  }
  // D: column = lane & 15 (ci), row = 4 * (lane >> 4) + register (co)
  float* out = part + (((long long)blockIdx.x * taps + t) * Cout) * Cin16;
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int n = 0; n < NBI; ++n) {
      const int ci = ci0 + 16 * n + j;
      const int co = co0 + 16 * m + 4 * g;
      out[(long long)(co + 0) * Cin16 + ci] = acc[m][n].x;
      out[(long long)(co + 1) * Cin16 + ci] = acc[m][n].y;
      out[(long long)(co + 2) * Cin16 + ci] = acc[m][n].z;
      out[(long long)(co + 3) * Cin16 + ci] = acc[m][n].w;
    }
}

// the splits in index order; one thread per real (tap, co, ci). OIDHW [Cout][Cin][taps], or IODHW [Cin][Cout][taps]
__global__ __launch_bounds__(256) void conv3d_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                                  int nsplit, int taps, int Cout_pad, int Cin16,
                                                                  int Cout, int Cin, int iodhw, int accumulate,
                                                                  long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ci = (int)(i % Cin), co = (int)((i / Cin) % Cout), t = (int)(i / ((long long)Cin * Cout));
  const long long stride = (long long)taps * Cout_pad * Cin16;
  const float* p = part + ((long long)t * Cout_pad + co) * Cin16 + ci;
  float s = 0.f;
  for (int k = 0; k < nsplit; ++k) s += p[k * stride];
  float* o = dw + (iodhw ? ((long long)ci * Cout + co) * taps + t : ((long long)co * Cin + ci) * taps + t);
  *o = accumulate ? *o + s : s;
}

int wgrad_plan(const char* what, int dtype, int N, int D, int H, int W, int Cin, int Cout, int ks, int deconv,
               long long* nvox, long long* per, int* nsplit, long long* bytes) {
  const int rc = t3_rows(what, dtype, N, D, H, W, nvox);
  if (rc != HR_OK) return rc;
  HR_REQUIRE(t3_channels_ok(Cin, Cout), "%s: Cin = %d (a multiple of 4, 4..4096), Cout = %d (a multiple of 16, 16..4096)",
             what, Cin, Cout);
  if (deconv) {
    HR_REQUIRE(ks == 2, "%s: ks = %d (the deconvolution is 2)", what, ks);
    HR_REQUIRE(*nvox * 8 <= kMaxVox, "%s: %lld output voxels (at most 2^36)", what, *nvox * 8);
  } else {
    HR_REQUIRE(ks == 1 || ks == 3 || ks == 7, "%s: ks = %d (1, 3 or 7)", what, ks);
  }
  long long s = (*nvox + kSplitVox - 1) / kSplitVox;
  if (s > kMaxSplits) s = kMaxSplits;
  long long p = (*nvox + s - 1) / s;
  p = (p + 15) / 16 * 16;                            // whole steps of 16 voxels
  *per = p;
  *nsplit = (int)((*nvox + p - 1) / p);
  const int Cin16 = (Cin + 15) / 16 * 16;
  *bytes = (long long)*nsplit * ks * ks * ks * Cout * Cin16 * (long long)sizeof(float);   // < 256 * 343 * 2^24 * 4: fits
  return HR_OK;
}

}  // namespace

extern "C" int hrnet_bn3d_parts(long long rows) { return rows >= 1 ? bn_parts(rows) : 0; }

extern "C" int hrnet_bn3d_stats(int dtype, const void* z, const float* gamma, const float* beta, float* scratch,
                                float* mean, float* invstd, float* scale, float* shift, float* running_mean,
                                float* running_var, long long* num_batches_tracked, int N, int D, int H, int W, int C,
                                int Creal, float momentum, float eps, hr_stream_t stream) {
  long long rows = 0;
  const int rc = t3_rows("bn3d_stats", dtype, N, D, H, W, &rows);
  if (rc != HR_OK) return rc;
  HR_REQUIRE(C >= 16 && C % 16 == 0 && C <= kBnMaxC && Creal >= 1 && Creal <= C,
             "bn3d_stats: C = %d (a multiple of 16, 16..%d), of which %d are real", C, kBnMaxC, Creal);
  HR_REQUIRE(rows >= 2, "bn3d_stats: Expected more than 1 value per channel when training (N * D * H * W = %lld)", rows);
  HR_REQUIRE(z && scratch && mean && invstd && scale && shift, "bn3d_stats: null argument");
  HR_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn3d_stats: one running statistic without the other");
  HR_REQUIRE(momentum >= 0.f && momentum <= 1.f && eps > 0.f, "bn3d_stats: momentum = %g, eps = %g", momentum, eps);
  const int parts = bn_parts(rows);
  const long long per = (rows + parts - 1) / parts;
  float* psum = scratch;
  float* psq = scratch + (long long)parts * C;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bn3d_sums_kernel<0>, dim3(parts), dim3(kBnThreads), 0, s, (const float*)z, nullptr, nullptr, nullptr,
                     nullptr, nullptr, nullptr, nullptr, psum, nullptr, rows, C, per, parts);
  hipLaunchKernelGGL(bn3d_sums_kernel<1>, dim3(parts), dim3(kBnThreads), 0, s, (const float*)z, nullptr, nullptr, nullptr,
                     nullptr, nullptr, nullptr, psum, psq, nullptr, rows, C, per, parts);
  hipLaunchKernelGGL(bn3d_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0, s, psum, psq, parts, gamma, beta, mean, invstd,
                     scale, shift, running_mean, running_var, num_batches_tracked, (double)rows, momentum, eps, C, Creal);
  return hr_check_launch("bn3d_stats");
}

extern "C" int hrnet_bn3d_apply(int dtype, const void* z, const float* scale, const float* shift, const void* other,
                                void* y, int N, int D, int H, int W, int C, int relu, int other_after_relu,
                                hr_stream_t stream) {
  long long rows = 0;
  const int rc = t3_rows("bn3d_apply", dtype, N, D, H, W, &rows);
  if (rc != HR_OK) return rc;
  HR_REQUIRE(C >= 4 && C % 4 == 0 && C <= 4096, "bn3d_apply: C = %d (a multiple of 4, 4..4096)", C);
  HR_REQUIRE(z && scale && shift && y, "bn3d_apply: null argument");
  HR_REQUIRE(other != y, "bn3d_apply: y aliases the added tensor");
  const long long total = rows * (C / 4);
  HR_REQUIRE(total <= 0xffffffffLL * 256, "bn3d_apply: %lld elements (at most 2^42)", total * 4);
  hipLaunchKernelGGL(bn3d_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)z, scale, shift, (const float*)other, (float*)y, total, C, relu != 0,
                     other_after_relu != 0);
  return hr_check_launch("bn3d_apply");
}

extern "C" int hrnet_bn3d_bwd(int dtype, const void* dy, const void* z, const void* mask_y, const float* scale,
                              const float* shift, const float* mean, const float* invstd, float* scratch, void* dz,
                              void* dother, float* dgamma, float* dbeta, float* dbias, int N, int D, int H, int W, int C,
                              int Creal, int recompute_mask, int accumulate_other, int accumulate_params,
                              hr_stream_t stream) {
  long long rows = 0;
  const int rc = t3_rows("bn3d_bwd", dtype, N, D, H, W, &rows);
  if (rc != HR_OK) return rc;
  HR_REQUIRE(C >= 16 && C % 16 == 0 && C <= kBnMaxC && Creal >= 1 && Creal <= C,
             "bn3d_bwd: C = %d (a multiple of 16, 16..%d), of which %d are real", C, kBnMaxC, Creal);
  HR_REQUIRE(dy && scratch, "bn3d_bwd: null argument");
  const bool has_bn = z != nullptr;
  if (has_bn) {
    HR_REQUIRE(scale && shift && mean && invstd && dz, "bn3d_bwd: null argument");
    HR_REQUIRE(dz != dy && dz != z && dz != mask_y && dother != dz && dother != dy, "bn3d_bwd: dz or dother aliases an input");
    HR_REQUIRE(!(mask_y && recompute_mask), "bn3d_bwd: a saved output and a recomputed mask, both");
  } else {
    HR_REQUIRE(!dz && !dother && !mask_y && !recompute_mask && !dgamma && !dbeta,
               "bn3d_bwd: without z (no BatchNorm) only the bias sum is formed");
  }
  const long long total = rows * (C / 4);
  HR_REQUIRE(total <= 0xffffffffLL * 256, "bn3d_bwd: %lld elements (at most 2^42)", total * 4);
  const int parts = bn_parts(rows);
  const long long per = (rows + parts - 1) / parts;
  float* pg = scratch;
  float* pgx = scratch + (long long)parts * C;
  float* coef = scratch + 2LL * parts * C;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bn3d_sums_kernel<2>, dim3(parts), dim3(kBnThreads), 0, s, (const float*)z, (const float*)dy,
                     (const float*)mask_y, recompute_mask ? scale : nullptr, shift, mean, invstd, nullptr, pg, pgx, rows,
                     C, per, parts);
  hipLaunchKernelGGL(bn3d_bwd_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0, s, pg, pgx, parts, (double)rows,
                     has_bn ? coef : nullptr, dgamma, dbeta, dbias, C, Creal, has_bn ? 1 : 0, accumulate_params != 0);
  if (has_bn) {
    hipLaunchKernelGGL(bn3d_bwd_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)dy,
                       (const float*)z, (const float*)mask_y, scale, shift, mean, invstd, coef, (float*)dz,
                       (float*)dother, total, C, recompute_mask != 0, accumulate_other != 0);
  }
  return hr_check_launch("bn3d_bwd");
}

extern "C" int hrnet_maxpool3d_bwd(int dtype, const void* x, const void* dy, void* dx, int N, int D, int H, int W, int C,
                                   int accumulate, hr_stream_t stream) {
  HR_REQUIRE(dtype == HR_F32, "maxpool3d_bwd: dtype = %d: only f32 (HR_F32 = 0) is built", dtype);
  HR_REQUIRE(x && dy && dx && dx != x && dx != dy, "maxpool3d_bwd: null or aliased argument");
  HR_REQUIRE(N >= 1 && D >= 2 && H >= 2 && W >= 2 && C >= 4 && C % 4 == 0 && C <= 4096,
             "maxpool3d_bwd: N = %d, D = %d, H = %d, W = %d, C = %d (a multiple of 4, 4..4096)", N, D, H, W, C);
  HR_REQUIRE(D % 2 == 0 && H % 2 == 0 && W % 2 == 0, "maxpool3d_bwd: D = %d, H = %d, W = %d must be even", D, H, W);
  const long long nvox = t3_product(N, D / 2, H / 2, W / 2);
  HR_REQUIRE(nvox <= kMaxVox, "maxpool3d_bwd: more than 2^36 output voxels (N = %d, D = %d, H = %d, W = %d)", N, D, H, W);
  const long long total = nvox * (C / 4);
  HR_REQUIRE(total <= 0xffffffffLL * 256, "maxpool3d_bwd: %lld outputs (at most 2^42)", total * 4);
  hipLaunchKernelGGL(maxpool3d_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)x, (const float*)dy, (float*)dx, total, D / 2, H / 2, W / 2, C, accumulate != 0);
  return hr_check_launch("maxpool3d_bwd");
}

extern "C" int hrnet_pack_weights3d_dgrad(int dtype, const float* w, void* out, int Cout, int Cin, int ks, int Cout_pad,
                                          int Cin_pad, hr_stream_t stream) {
  HR_REQUIRE(dtype == HR_F32, "pack_weights3d_dgrad: dtype = %d: only f32 (HR_F32 = 0) is built", dtype);
  HR_REQUIRE(w && out, "pack_weights3d_dgrad: null argument");
  HR_REQUIRE(ks == 1 || ks == 3 || ks == 7, "pack_weights3d_dgrad: ks = %d (1, 3 or 7)", ks);
  // the roles are exchanged: Cin_pad is the output side of the input-gradient convolution (a multiple of 16)
  HR_REQUIRE(Cout >= 1 && Cin >= 1 && Cout_pad >= Cout && Cin_pad >= Cin && t3_channels_ok(Cout_pad, Cin_pad),
             "pack_weights3d_dgrad: Cout = %d in %d, Cin = %d in %d (pads: multiples of 4 and of 16)", Cout, Cout_pad, Cin,
             Cin_pad);
  const int taps = ks * ks * ks;
  const long long total = (long long)taps * Cout_pad * Cin_pad;
  hipLaunchKernelGGL(pack_weights3d_dgrad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     w, (float*)out, Cout, Cin, taps, Cout_pad, Cin_pad, total);
  return hr_check_launch("pack_weights3d_dgrad");
}

extern "C" int hrnet_deconv3d_k2s2_dgrad(int dtype, const void* dz, const void* w_packed, void* dx, int N, int D, int H,
                                         int W, int Cin, int Cout, int accumulate, hr_stream_t stream) {
  long long nvox = 0;
  const int rc = t3_rows("deconv3d_k2s2_dgrad", dtype, N, D, H, W, &nvox);
  if (rc != HR_OK) return rc;
  HR_REQUIRE(Cin >= 16 && Cin % 16 == 0 && Cin <= 4096 && Cout >= 16 && Cout % 16 == 0 && Cout <= 4096,
             "deconv3d_k2s2_dgrad: Cin = %d, Cout = %d (multiples of 16, 16..4096)", Cin, Cout);
  HR_REQUIRE(nvox * 8 <= kMaxVox, "deconv3d_k2s2_dgrad: %lld output voxels (at most 2^36)", nvox * 8);
  HR_REQUIRE(dz && w_packed && dx && dx != dz, "deconv3d_k2s2_dgrad: null or aliased argument");
  const int nb = Cin % 64 == 0 ? 4 : (Cin % 32 == 0 ? 2 : 1);
  const dim3 grid((unsigned)((nvox + kBlockVox - 1) / kBlockVox), (unsigned)(Cin / (16 * nb)));
#define T3_GO(NB)                                                                                                  \
  hipLaunchKernelGGL((deconv3d_dgrad_kernel<NB>), grid, dim3(64 * kWaves), 0, (hipStream_t)stream, (const float*)dz, \
                     (const float*)w_packed, (float*)dx, nvox, D, H, W, Cin, Cout, accumulate != 0)
  if (nb == 4) T3_GO(4); else if (nb == 2) T3_GO(2); else T3_GO(1);
#undef T3_GO
  return hr_check_launch("deconv3d_k2s2_dgrad");
}

extern "C" int hrnet_conv3d_wgrad_scratch(int dtype, int N, int D, int H, int W, int Cin, int Cout, int ks, int deconv,
                                          long long* bytes, int* nsplit, long long* split_voxels) {
  HR_REQUIRE(bytes && nsplit, "conv3d_wgrad_scratch: null argument");
  long long nvox = 0, per = 0;
  const int rc = wgrad_plan("conv3d_wgrad_scratch", dtype, N, D, H, W, Cin, Cout, ks, deconv, &nvox, &per, nsplit, bytes);
  if (rc == HR_OK && split_voxels) *split_voxels = per;
  return rc;
}

extern "C" int hrnet_conv3d_wgrad(int dtype, const void* x, const void* dz, void* scratch, long long scratch_bytes,
                                  float* dw, int N, int D, int H, int W, int Cin, int Cout, int Cin_real, int Cout_real,
                                  int ks, int deconv, int accumulate, hr_stream_t stream) {
  long long nvox = 0, per = 0, bytes = 0;
  int nsplit = 0;
  const int rc = wgrad_plan("conv3d_wgrad", dtype, N, D, H, W, Cin, Cout, ks, deconv, &nvox, &per, &nsplit, &bytes);
  if (rc != HR_OK) return rc;
  HR_REQUIRE(Cin_real >= 1 && Cin_real <= Cin && Cout_real >= 1 && Cout_real <= Cout,
             "conv3d_wgrad: %d real of Cin = %d, %d real of Cout = %d", Cin_real, Cin, Cout_real, Cout);
  HR_REQUIRE(x && dz && scratch && dw, "conv3d_wgrad: null argument");
  HR_REQUIRE(scratch_bytes >= bytes, "conv3d_wgrad: scratch of %lld bytes, %lld needed (hrnet_conv3d_wgrad_scratch)",
             scratch_bytes, bytes);
  const int taps = ks * ks * ks;
  const int Cin16 = (Cin + 15) / 16 * 16;
  const int mb = Cout % 32 == 0 ? 2 : 1, nbi = Cin16 % 32 == 0 ? 2 : 1;
  const int ci_blocks = Cin16 / (16 * nbi), co_blocks = Cout / (16 * mb);
  HR_REQUIRE((long long)ci_blocks * co_blocks <= 65535, "conv3d_wgrad: %d x %d channel blocks (at most 65535)", co_blocks,
             ci_blocks);
  const dim3 grid((unsigned)nsplit, (unsigned)taps, (unsigned)(ci_blocks * co_blocks));
  const hipStream_t s = (hipStream_t)stream;
#define T3_WG(MB, NBI, DC)                                                                                           \
  hipLaunchKernelGGL((conv3d_wgrad_kernel<MB, NBI, DC>), grid, dim3(64), 0, s, (const float*)x, (const float*)dz,      \
                     (float*)scratch, nvox, per, D, H, W, Cin, Cout, Cin16, ks, ci_blocks)
  if (deconv) {
    if (mb == 2 && nbi == 2) T3_WG(2, 2, true); else if (mb == 2) T3_WG(2, 1, true);
    else if (nbi == 2) T3_WG(1, 2, true); else T3_WG(1, 1, true);
  } else {
    if (mb == 2 && nbi == 2) T3_WG(2, 2, false); else if (mb == 2) T3_WG(2, 1, false);
    else if (nbi == 2) T3_WG(1, 2, false); else T3_WG(1, 1, false);
  }
#undef T3_WG
  const long long total = (long long)taps * Cout_real * Cin_real;
  hipLaunchKernelGGL(conv3d_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     (const float*)scratch, dw, nsplit, taps, Cout, Cin16, Cout_real, Cin_real, deconv != 0,
                     accumulate != 0, total);
  return hr_check_launch("conv3d_wgrad");
}
