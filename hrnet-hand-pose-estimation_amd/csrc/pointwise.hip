// 1x1 convolution on NCHW f32, forward and backward: process_features of the volumetric model (reference
// lib/models/triangulation.py:345-349), Conv2d(480, 32, 1) between the backbone's NCHW concatenation and the
// unprojection, which takes NCHW too. The weight is the module's own [Cout][Cin] tensor, read in place: nothing is packed.
// All contractions run on mfma_f32_16x16x4f32 (A: lane (i = l & 15, g = l >> 4) holds A[i][g], B: lane (j, g) holds
// B[g][j], D: column = l & 15, row = 4 * (l >> 4) + register). No atomics: every sum has one fixed order.
//
//   forward   y[n,o,p] = bias[o] + sum_c w[o,c] x[n,c,p]. Rows = output channels, columns = pixels, K = channels. Pixels
//             are the contiguous axis, so a lane loads FOUR consecutive pixels of one channel with one 16-byte load: lane
//             (j, g) reads pixels p0 + 4j .. 4j + 3 of channel c0 + 4g + t, 16 lanes cover 256 contiguous bytes of a row.
//             Component q of that vector is column j of pixel group q (pixel p0 + 4j + q), so a wave owns 64 pixels as
//             4 groups x ceil(Cout / 16) accumulators, and a lane ends up with 4 consecutive pixels of each of its rows:
//             the store is a 16-byte vector as well. The weight fragment of 16 channels is one 16-byte load per lane,
//             (row j, channels c0 + 4g .. 4g + 3), the same k order as x. Every x element is loaded once, by one lane.
//             The weights are read through L1/L2, not staged in LDS ("The vol model", has the comparison).
//   dx        dx[n,c,p] = sum_o w[o,c] dy[n,o,p]. Rows = input channels, columns = pixels, K = Cout: a wave keeps the dy
//             of its 64 pixels in registers and walks the input channels 16 at a time.
//   dw, db    dw[o,c] = sum_{n,p} dy[n,o,p] x[n,c,p]. Rows = o, columns = c, K = pixels: lane (j, g) loads pixels
//             p0 + 4g .. 4g + 3 of row j. A wave owns one part of the (n, 16-pixel tile) sequence and 64 input channels
//             and writes its sums into row `part` of the scratch; db is the same MFMA against ones. A second launch adds
//             the rows in index order.
// Tails: pixels >= P, channels >= Cin and outputs >= Cout are loaded as zeros (never dereferenced) and not stored, so
// every MFMA runs with all 64 lanes on. The 16-byte paths need P % 4 == 0 (Cin % 4 == 0 for w) and aligned pointers;
// anything else takes the element-wise loads of the same kernels.
#include "common.h"

namespace {

constexpr int kWavePix = 64;           // pixels of one wave: 16 lanes x 4
constexpr int kMaxWaves = 4;
constexpr int kMaxCout = 64;
constexpr int kMaxCin = 1 << 16;
constexpr int kMaxN = 65535;           // grid.y
constexpr long long kMaxP = 1LL << 30;
constexpr long long kMaxElems = 1LL << 40;
constexpr int kPartTiles = 32;         // 16-pixel tiles of one part of the weight gradient, until kMaxParts are in use
constexpr int kMaxParts = 256;
constexpr int kChunk = 64;             // input channels of one weight-gradient wave

// four consecutive pixels of one row, zeros beyond P
template <bool VEC>
__device__ __forceinline__ f32x4 load_px(const float* __restrict__ row, long long p, long long P) {
  if (VEC) return p < P ? *(const f32x4*)(row + p) : f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 v;
  v.x = p < P ? row[p] : 0.f;
  v.y = p + 1 < P ? row[p + 1] : 0.f;
  v.z = p + 2 < P ? row[p + 2] : 0.f;
  v.w = p + 3 < P ? row[p + 3] : 0.f;
  return v;
}

template <bool VEC>
__device__ __forceinline__ void store_px(float* __restrict__ row, long long p, long long P, const f32x4& v) {
  if (VEC) {
    if (p < P) *(f32x4*)(row + p) = v;
    return;
  }
  if (p < P) row[p] = v.x;
  if (p + 1 < P) row[p + 1] = v.y;
  if (p + 2 < P) row[p + 2] = v.z;
  if (p + 3 < P) row[p + 3] = v.w;
}

// w[o][c .. c + 3], zeros beyond Cout and Cin; vec (wave-uniform): Cin % 4 == 0 and w is 16-byte aligned
__device__ __forceinline__ f32x4 load_w4(const float* __restrict__ w, int o, int c, int Cin, int Cout, bool vec) {
  if (o >= Cout || c >= Cin) return f32x4{0.f, 0.f, 0.f, 0.f};
  const float* r = w + (long long)o * Cin + c;
  if (vec) return *(const f32x4*)r;
  f32x4 v;
  v.x = r[0];
  v.y = c + 1 < Cin ? r[1] : 0.f;
  v.z = c + 2 < Cin ? r[2] : 0.f;
  v.w = c + 3 < Cin ? r[3] : 0.f;
  return v;
}

#define PW_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

template <int NB, bool XVEC>
__global__ __launch_bounds__(64 * kMaxWaves) void pw_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float* __restrict__ y,
                                                                int Cin, int Cout, long long P, int tiles,
                                                                int wvec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const float* xn = x + (long long)blockIdx.y * Cin * P;
  float* yn = y + (long long)blockIdx.y * Cout * P;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long p0 = ((long long)tile * waves + wave) * kWavePix;
    if (p0 >= P) continue;                       // the whole wave
    const long long p = p0 + 4 * j;
    f32x4 acc[4][NB];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int n = 0; n < NB; ++n) acc[q][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < Cin; c0 += 16) {
      f32x4 a[NB], b[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int c = c0 + 4 * g + t;
        b[t] = c < Cin ? load_px<XVEC>(xn + (long long)c * P, p, P) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int n = 0; n < NB; ++n) a[n] = load_w4(w, n * 16 + j, c0 + 4 * g, Cin, Cout, wvec != 0);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int n = 0; n < NB; ++n) acc[q][n] = PW_MFMA(a[n][t], b[t][q], acc[q][n]);
    }
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = n * 16 + 4 * g + r;
        if (o >= Cout) continue;
        const float bo = bias ? bias[o] : 0.f;
        const f32x4 v = {acc[0][n][r] + bo, acc[1][n][r] + bo, acc[2][n][r] + bo, acc[3][n][r] + bo};
        store_px<XVEC>(yn + (long long)o * P, p, P, v);
      }
  }
}

template <int NB, bool XVEC>
__global__ __launch_bounds__(64 * kMaxWaves) void pw_dx_kernel(const float* __restrict__ w, const float* __restrict__ dy,
                                                               float* __restrict__ dx, int Cin, int Cout, long long P,
                                                               int tiles) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const float* dyn = dy + (long long)blockIdx.y * Cout * P;
  float* dxn = dx + (long long)blockIdx.y * Cin * P;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long p0 = ((long long)tile * waves + wave) * kWavePix;
    if (p0 >= P) continue;                       // the whole wave
    const long long p = p0 + 4 * j;
    f32x4 b[4 * NB];                             // k step s: output channel 4s + g
#pragma unroll
    for (int s = 0; s < 4 * NB; ++s) {
      const int o = 4 * s + g;
      b[s] = o < Cout ? load_px<XVEC>(dyn + (long long)o * P, p, P) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int c0 = 0; c0 < Cin; c0 += 16) {
      float a[4 * NB];
#pragma unroll
      for (int s = 0; s < 4 * NB; ++s) {
        const int o = 4 * s + g;
        a[s] = (o < Cout && c0 + j < Cin) ? w[(long long)o * Cin + c0 + j] : 0.f;
      }
      f32x4 acc[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 4 * NB; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = PW_MFMA(a[s], b[s][q], acc[q]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = c0 + 4 * g + r;
        if (c >= Cin) continue;
        const f32x4 v = {acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
        store_px<XVEC>(dxn + (long long)c * P, p, P, v);
      }
    }
  }
}

// one wave: part blockIdx.x of the tiles, input channels [64 * blockIdx.y, +64)
template <int NB, bool XVEC>
__global__ __launch_bounds__(64) void pw_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                      float* __restrict__ scratch, int Cin, int Cout, long long P,
                                                      long long tiles_per_n, long long tiles, long long per) {
  constexpr int CB = kChunk / 16;
  const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
  const int cbase = blockIdx.y * kChunk;
  const bool first = blockIdx.y == 0;
  f32x4 acc[CB][NB], accb[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    accb[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) acc[cb][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const long long t0 = (long long)blockIdx.x * per;
  const long long t1 = t0 + per < tiles ? t0 + per : tiles;
  for (long long tile = t0; tile < t1; ++tile) {
    const long long n = tile / tiles_per_n;
    const long long p = (tile - n * tiles_per_n) * 16 + 4 * g;
    f32x4 a[NB], b[CB];
#pragma unroll
    for (int m = 0; m < NB; ++m) {
      const int o = m * 16 + j;
      a[m] = o < Cout ? load_px<XVEC>(dy + (n * Cout + o) * P, p, P) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      const int c = cbase + cb * 16 + j;
      b[cb] = c < Cin ? load_px<XVEC>(x + (n * Cin + c) * P, p, P) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int m = 0; m < NB; ++m) acc[cb][m] = PW_MFMA(a[m][t], b[cb][t], acc[cb][m]);
    if (first) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int m = 0; m < NB; ++m) accb[m] = PW_MFMA(a[m][t], 1.f, accb[m]);
    }
  }
  float* row = scratch + (long long)blockIdx.x * ((long long)Cout * Cin + Cout);
#pragma unroll
  for (int m = 0; m < NB; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = m * 16 + 4 * g + r;
      if (o >= Cout) continue;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const int c = cbase + cb * 16 + j;
        if (c < Cin) row[(long long)o * Cin + c] = acc[cb][m][r];
      }
      if (first && j == 0) row[(long long)Cout * Cin + o] = accb[m][r];
    }
}

// dw[e] / db[e - Cout * Cin] = the scratch rows added in index order
__global__ __launch_bounds__(256) void pw_wgrad_reduce_kernel(const float* __restrict__ scratch, float* __restrict__ dw,
                                                              float* __restrict__ db, int parts, long long nw,
                                                              long long rowlen) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= rowlen) return;
  if (e < nw ? dw == nullptr : db == nullptr) return;
  float s = 0.f;
  for (int r = 0; r < parts; ++r) s += scratch[(long long)r * rowlen + e];
  if (e < nw)
    dw[e] = s;
  else
    db[e - nw] = s;
}

long long pw_tiles(int N, long long P) { return (long long)N * ((P + 15) / 16); }

long long pw_per_part(long long tiles) {
  long long per = kPartTiles;
  if ((tiles + per - 1) / per > kMaxParts) per = (tiles + kMaxParts - 1) / kMaxParts;
  return per;
}

int pw_shape(const char* what, int dtype, int N, int Cin, int Cout, long long P) {
  HR_REQUIRE(dtype == HR_F32, "%s: dtype = %d: only f32 (HR_F32 = 0) is built", what, dtype);
  HR_REQUIRE(hrnet_pointwise_nchw_supported(dtype, Cin, Cout), "%s: Cin = %d, Cout = %d: needs 1 <= Cin <= %d and "
             "1 <= Cout <= %d", what, Cin, Cout, kMaxCin, kMaxCout);
  HR_REQUIRE(N >= 1 && N <= kMaxN && P >= 1 && P <= kMaxP, "%s: N = %d, P = %lld: needs 1 <= N <= %d and 1 <= P <= 2^30",
             what, N, P, kMaxN);
  HR_REQUIRE((long long)N * P <= kMaxElems / (Cin > Cout ? Cin : Cout), "%s: N * P * max(Cin, Cout) = more than 2^40 "
             "elements (N = %d, P = %lld, Cin = %d, Cout = %d)", what, N, P, Cin, Cout);
  return HR_OK;
}

bool pw_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// waves of a workgroup: as many as keep at least two workgroups per compute unit busy
int pw_waves(int N, long long P) {
  for (int wv = kMaxWaves; wv > 1; wv >>= 1)
    if ((long long)N * ((P + wv * kWavePix - 1) / (wv * kWavePix)) >= 512) return wv;
  return 1;
}

template <int NB>
void pw_fwd_launch(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, long long P,
                   hipStream_t s) {
  const bool xvec = P % 4 == 0 && pw_aligned(x) && pw_aligned(y);
  const int wvec = Cin % 4 == 0 && pw_aligned(w);
  const int waves = pw_waves(N, P);
  const long long tiles = (P + waves * kWavePix - 1) / (waves * kWavePix);
  const dim3 grid((unsigned)(tiles > (1 << 20) ? (1 << 20) : tiles), (unsigned)N);
  if (xvec)
    pw_fwd_kernel<NB, true><<<grid, 64 * waves, 0, s>>>(x, w, bias, y, Cin, Cout, P, (int)tiles, wvec);
  else
    pw_fwd_kernel<NB, false><<<grid, 64 * waves, 0, s>>>(x, w, bias, y, Cin, Cout, P, (int)tiles, wvec);
}

template <int NB>
void pw_bwd_launch(const float* x, const float* w, const float* dy, float* dx, float* scratch, bool wgrad, int N,
                   int Cin, int Cout, long long P, hipStream_t s) {
  if (dx) {
    const bool vec = P % 4 == 0 && pw_aligned(dy) && pw_aligned(dx);
    const int waves = pw_waves(N, P);
    const long long tiles = (P + waves * kWavePix - 1) / (waves * kWavePix);
    const dim3 grid((unsigned)(tiles > (1 << 20) ? (1 << 20) : tiles), (unsigned)N);
    if (vec)
      pw_dx_kernel<NB, true><<<grid, 64 * waves, 0, s>>>(w, dy, dx, Cin, Cout, P, (int)tiles);
    else
      pw_dx_kernel<NB, false><<<grid, 64 * waves, 0, s>>>(w, dy, dx, Cin, Cout, P, (int)tiles);
  }
  if (wgrad) {
    const bool vec = P % 4 == 0 && pw_aligned(dy) && pw_aligned(x);
    const long long tiles = pw_tiles(N, P), per = pw_per_part(tiles);
    const dim3 grid((unsigned)((tiles + per - 1) / per), (unsigned)((Cin + kChunk - 1) / kChunk));
    if (vec)
      pw_wgrad_kernel<NB, true><<<grid, 64, 0, s>>>(x, dy, scratch, Cin, Cout, P, (P + 15) / 16, tiles, per);
    else
      pw_wgrad_kernel<NB, false><<<grid, 64, 0, s>>>(x, dy, scratch, Cin, Cout, P, (P + 15) / 16, tiles, per);
  }
}

}  // namespace

extern "C" int hrnet_pointwise_nchw_supported(int dtype, int Cin, int Cout) {
  return dtype == HR_F32 && Cin >= 1 && Cin <= kMaxCin && Cout >= 1 && Cout <= kMaxCout;
}

extern "C" int hrnet_pointwise_nchw_parts(int N, long long P) {
  if (N < 1 || N > kMaxN || P < 1 || P > kMaxP) return 0;
  const long long tiles = pw_tiles(N, P), per = pw_per_part(tiles);
  return (int)((tiles + per - 1) / per);
}

extern "C" int hrnet_pointwise_nchw(int dtype, const float* x, const float* w, const float* bias, float* y, int N,
                                    int Cin, int Cout, long long P, hr_stream_t stream) {
  if (const int rc = pw_shape("pointwise_nchw", dtype, N, Cin, Cout, P)) return rc;
  HR_REQUIRE(x && w && y, "pointwise_nchw: null pointer (x = %p, w = %p, y = %p)", (const void*)x, (const void*)w,
             (void*)y);
  HR_REQUIRE((const void*)x != (const void*)y, "pointwise_nchw: y aliases x");
  hipStream_t s = (hipStream_t)stream;
  switch ((Cout + 15) / 16) {
    case 1: pw_fwd_launch<1>(x, w, bias, y, N, Cin, Cout, P, s); break;
    case 2: pw_fwd_launch<2>(x, w, bias, y, N, Cin, Cout, P, s); break;
    case 3: pw_fwd_launch<3>(x, w, bias, y, N, Cin, Cout, P, s); break;
    default: pw_fwd_launch<4>(x, w, bias, y, N, Cin, Cout, P, s); break;
  }
  return hr_check_launch("pointwise_nchw");
}

extern "C" int hrnet_pointwise_nchw_bwd(int dtype, const float* x, const float* w, const float* dy, float* dx, float* dw,
                                        float* db, float* scratch, long long scratch_floats, int N, int Cin, int Cout,
                                        long long P, hr_stream_t stream) {
  if (const int rc = pw_shape("pointwise_nchw_bwd", dtype, N, Cin, Cout, P)) return rc;
  HR_REQUIRE(x && w && dy, "pointwise_nchw_bwd: null pointer (x = %p, w = %p, dy = %p)", (const void*)x, (const void*)w,
             (const void*)dy);
  HR_REQUIRE(dx || dw || db, "pointwise_nchw_bwd: dx, dw and db are all null: nothing to compute");
  HR_REQUIRE((const void*)dx != (const void*)dy && (const void*)dx != (const void*)x, "pointwise_nchw_bwd: dx aliases "
             "dy or x");
  const bool wgrad = dw || db;
  const int parts = hrnet_pointwise_nchw_parts(N, P);
  const long long rowlen = (long long)Cout * Cin + Cout;
  if (wgrad) {
    HR_REQUIRE(scratch, "pointwise_nchw_bwd: null scratch with dw or db asked for");
    HR_REQUIRE(scratch_floats >= parts * rowlen, "pointwise_nchw_bwd: scratch of %lld floats, %d rows of %lld are needed",
               scratch_floats, parts, rowlen);
  }
  hipStream_t s = (hipStream_t)stream;
  switch ((Cout + 15) / 16) {
    case 1: pw_bwd_launch<1>(x, w, dy, dx, scratch, wgrad, N, Cin, Cout, P, s); break;
    case 2: pw_bwd_launch<2>(x, w, dy, dx, scratch, wgrad, N, Cin, Cout, P, s); break;
    case 3: pw_bwd_launch<3>(x, w, dy, dx, scratch, wgrad, N, Cin, Cout, P, s); break;
    default: pw_bwd_launch<4>(x, w, dy, dx, scratch, wgrad, N, Cin, Cout, P, s); break;
  }
  if (wgrad)
    pw_wgrad_reduce_kernel<<<(unsigned)((rowlen + 255) / 256), 256, 0, s>>>(scratch, dw, db, parts, (long long)Cout * Cin,
                                                                           rowlen);
  return hr_check_launch("pointwise_nchw_bwd");
}
