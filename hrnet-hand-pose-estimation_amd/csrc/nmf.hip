// NMF kernels of pose_hrnet_hamburger, the reference's HamNet (lib/models/hamburger/ham.py, class NMF2D): the multiplicative
// update, the Gram matrix, the plain product and the reconstruction. f32 throughout, 64-bit element offsets, no float
// atomics: every sum has one fixed order, so a call is bit-reproducible.
//
// ONE engine, nmf_gemm_kernel, computes C[m, n] = sum_k A[m, k] B[k, n] for operands given by two element strides each, one
// of which is 1. A workgroup of 4 waves owns a 64 x 64 tile of C, a wave a 32 x 32 quarter as 2 x 2 tiles of
// mfma_f32_16x16x4f32 - or, when the launch would have fewer than 256 such workgroups and leave compute units idle (a
// (512, 512) update of one image is 64 tiles), a 32 x 32 tile with one MFMA tile per wave: four times the workgroups for
// twice the operand traffic per product. Layout of mfma_f32_16x16x4f32: A: lane (i = l & 15, g = l >> 4) holds A[i][g],
// B: lane (j, g) holds B[g][j], D: column = l & 15, row = 4 * (l >> 4) + register.
// The reduction runs in chunks of 16: the threads fetch a 16 x 64 (16 x 32) panel of each operand into registers (one
// float4 each when the operand allows it, four bounds-checked element loads otherwise, chosen per operand and uniform
// over the launch), the panels of the NEXT chunk are fetched while the MFMAs of this one run, and they meet in LDS as
// [k][64 + 16]: the row stride of 80 floats puts the four k rows that one MFMA operand reads on disjoint banks. Every 256
// reduction steps the accumulator is added into a second one and cleared, so that a sum of 4096 terms is 16 sums of 256
// and the rounding error grows with the square roots of both, not with 4096.
//
//   update     T' = T * (op(X) F) / (T Gm + eps): the engine runs twice into two accumulators - over K for the numerator,
//              over R for the denominator - and the ratio is taken on the registers; neither product reaches memory.
//   gram       Gm = A^T A; a long K is split over workgroups, the parts go to the caller's scratch and a second launch
//              adds them in split order.
//   product    op(X) F, and the reconstruction Bs Cf^T stored through a leading dimension in either orientation (the
//              engine computes whichever of the product and its transpose has unit column stride in memory).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "hrnet_hip.h"

namespace {

constexpr int kMaxDim = 1 << 24;       // largest M, K, R, D, N
constexpr int kMaxG = 65535;           // batch entries (times Gram splits) ride on grid.y
constexpr int kTile = 64;              // C tile of a workgroup ...
constexpr int kSmallTile = 32;         // ... and of a launch that would leave compute units idle with the large one
constexpr int kFillGrid = 256;         // workgroups of 64 x 64 tiles below which the 32 x 32 tile is taken (the CU count)
constexpr int kBK = 16;                // reduction chunk
constexpr int kLd = kTile + 16;        // LDS row stride
constexpr int kFlush = 16;             // chunks per partial sum (256 reduction steps)
constexpr int kGramTiles = 512;        // the Gram split aims at this many workgroups
constexpr int kGramMinK = 256;         // ... and at parts no shorter than this

typedef float nmf_f4 __attribute__((ext_vector_type(4)));
#define NMF_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

struct NmfOperand {      // element (i, k) of a panel operand sits at p[i * s_i + k * s_k] (+ batch * bs)
  const float* p;
  long long s_i, s_k, bs;
  int vec;               // 16-byte loads are legal
};

struct NmfGemm {
  NmfOperand a1, b1;     // numerator / plain product: A (M, K1), B (K1, N)
  NmfOperand a2, b2;     // denominator of the update: A = T (M, K2), B = Gm (K2, N); K2 = 0 otherwise
  const float* t;        // update: T (M, N) row-major, batch stride M * N
  float* c;
  long long c_sm, c_bs, c_ss;   // row stride (columns are contiguous), batch stride, split stride
  int M, N, K1, K2, tiles_n, splits, kchunk;
  float eps;
};

// a 16 x TILE panel is 4 TILE threads with 4 values each: every thread for TILE 64, the first 128 for TILE 32
template <int TILE>
__device__ __forceinline__ void nmf_fetch(const NmfOperand& o, const float* base, int i0, int k0, int I, int kend,
                                          int tid, float v[4]) {
  if (tid >= 4 * TILE) return;
  if (o.s_i == 1) {      // contiguous along the tile: thread = (k, 4 consecutive i)
    const int k = k0 + tid / (TILE / 4), i = i0 + (tid % (TILE / 4)) * 4;
    const float* q = base + (long long)k * o.s_k + i;
    if (o.vec && k < kend && i + 3 < I) {
      const float4 w = *reinterpret_cast<const float4*>(q);
      v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (k < kend && i + e < I) ? q[e] : 0.f;
    }
  } else {               // contiguous along the reduction: thread = (i, 4 consecutive k)
    const int i = i0 + (tid >> 2), k = k0 + (tid & 3) * 4;
    const float* q = base + (long long)i * o.s_i + (long long)k * o.s_k;
    if (o.vec && i < I && k + 3 < kend) {
      const float4 w = *reinterpret_cast<const float4*>(q);
      v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (i < I && k + e < kend) ? q[(long long)e * o.s_k] : 0.f;
    }
  }
}

template <int TILE>
__device__ __forceinline__ void nmf_stash(float (*S)[kLd], bool along_tile, int tid, const float v[4]) {
  if (tid >= 4 * TILE) return;
  if (along_tile) {
    *reinterpret_cast<float4*>(&S[tid / (TILE / 4)][(tid % (TILE / 4)) * 4]) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) S[(tid & 3) * 4 + e][tid >> 2] = v[e];
  }
}

// tot[i][j] = A[m0 + ..][kbeg .. kend) B[kbeg .. kend)[n0 + ..] for this wave's F x F MFMA tiles, F = TILE / 32: the four
// waves own the quarters of the TILE x TILE tile
template <int TILE>
__device__ __forceinline__ void nmf_reduce(const NmfOperand& a, const NmfOperand& b, long long batch, int m0, int n0, int M,
                                           int N, int kbeg, int kend, float (*As)[kLd], float (*Bs)[kLd],
                                           nmf_f4 tot[TILE / 32][TILE / 32]) {
  constexpr int F = TILE / 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * (TILE / 2), wn = (wave & 1) * (TILE / 2);
  const float* pa = a.p + batch * a.bs;
  const float* pb = b.p + batch * b.bs;
  const bool a_tile = a.s_i == 1, b_tile = b.s_i == 1;
  nmf_f4 acc[F][F];
#pragma unroll
  for (int i = 0; i < F; ++i)
#pragma unroll
    for (int j = 0; j < F; ++j) {
      acc[i][j] = (nmf_f4){0.f, 0.f, 0.f, 0.f};
      tot[i][j] = (nmf_f4){0.f, 0.f, 0.f, 0.f};
    }
  float va[4] = {0.f, 0.f, 0.f, 0.f}, vb[4] = {0.f, 0.f, 0.f, 0.f};
  if (kbeg < kend) {
    nmf_fetch<TILE>(a, pa, m0, kbeg, M, kend, tid, va);
    nmf_fetch<TILE>(b, pb, n0, kbeg, N, kend, tid, vb);
  }
  int chunk = 0;
  for (int k0 = kbeg; k0 < kend; k0 += kBK) {
    __syncthreads();                       // the MFMAs of the previous chunk have read the panels
    nmf_stash<TILE>(As, a_tile, tid, va);
    nmf_stash<TILE>(Bs, b_tile, tid, vb);
    __syncthreads();
    if (k0 + kBK < kend) {
      nmf_fetch<TILE>(a, pa, m0, k0 + kBK, M, kend, tid, va);
      nmf_fetch<TILE>(b, pb, n0, k0 + kBK, N, kend, tid, vb);
    }
#pragma unroll
    for (int kk = 0; kk < kBK / 4; ++kk) {
      const int kr = kk * 4 + (lane >> 4);
      float fa[F], fb[F];
#pragma unroll
      for (int i = 0; i < F; ++i) {
        fa[i] = As[kr][wm + i * 16 + (lane & 15)];
        fb[i] = Bs[kr][wn + i * 16 + (lane & 15)];
      }
#pragma unroll
      for (int i = 0; i < F; ++i)
#pragma unroll
        for (int j = 0; j < F; ++j) acc[i][j] = NMF_MFMA(fa[i], fb[j], acc[i][j]);
    }
    if (++chunk == kFlush) {
      chunk = 0;
#pragma unroll
      for (int i = 0; i < F; ++i)
#pragma unroll
        for (int j = 0; j < F; ++j) {
          tot[i][j] += acc[i][j];
          acc[i][j] = (nmf_f4){0.f, 0.f, 0.f, 0.f};
        }
    }
  }
#pragma unroll
  for (int i = 0; i < F; ++i)
#pragma unroll
    for (int j = 0; j < F; ++j) tot[i][j] += acc[i][j];
}

template <bool UPDATE, int TILE>
__global__ __launch_bounds__(256) void nmf_gemm_kernel(const NmfGemm g) {
  constexpr int F = TILE / 32;
  __shared__ __attribute__((aligned(16))) float As[kBK][kLd];
  __shared__ __attribute__((aligned(16))) float Bs[kBK][kLd];
  const int m0 = (int)(blockIdx.x / (unsigned)g.tiles_n) * TILE, n0 = (int)(blockIdx.x % (unsigned)g.tiles_n) * TILE;
  const long long batch = blockIdx.y / (unsigned)g.splits;
  const int split = (int)(blockIdx.y % (unsigned)g.splits);
  const int kbeg = split * g.kchunk;
  const int kend = g.K1 - kbeg < g.kchunk ? g.K1 : kbeg + g.kchunk;
  nmf_f4 num[F][F];
  nmf_reduce<TILE>(g.a1, g.b1, batch, m0, n0, g.M, g.N, kbeg, kend, As, Bs, num);
  nmf_f4 den[F][F];
  if (UPDATE) nmf_reduce<TILE>(g.a2, g.b2, batch, m0, n0, g.M, g.N, 0, g.K2, As, Bs, den);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* c = g.c + batch * g.c_bs + (long long)split * g.c_ss;
  const float* t = UPDATE ? g.t + batch * (long long)g.M * g.N : nullptr;
#pragma unroll
  for (int i = 0; i < F; ++i)
#pragma unroll
    for (int j = 0; j < F; ++j) {
      const int col = n0 + (wave & 1) * (TILE / 2) + j * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + (wave >> 1) * (TILE / 2) + i * 16 + 4 * (lane >> 4) + r;
        if (row < g.M && col < g.N) {
          float v = num[i][j][r];
          if (UPDATE) v = t[(long long)row * g.N + col] * v / (den[i][j][r] + g.eps);
          c[(long long)row * g.c_sm + col] = v;
        }
      }
    }
}

// Gm[g][i] = sum over the splits, in split order, of parts[g][s][i]
__global__ __launch_bounds__(256) void nmf_gram_reduce_kernel(const float* parts, float* out, long long rr, int splits,
                                                              long long total) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long b = i / rr, e = i - b * rr;
    const float* p = parts + b * splits * rr + e;
    float s = p[0];
    for (int k = 1; k < splits; ++k) s += p[(long long)k * rr];
    out[i] = s;
  }
}

bool nmf_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

NmfOperand nmf_operand(const float* p, long long s_i, long long s_k, long long bs) {
  NmfOperand o;
  o.p = p; o.s_i = s_i; o.s_k = s_k; o.bs = bs;
  const bool strides = s_i == 1 ? (s_k % 4 == 0) : (s_k == 1 && s_i % 4 == 0);
  o.vec = nmf_al16(p) && bs % 4 == 0 && strides;
  return o;
}

// the strided feature matrix read as op(X) (I, K): xt = 0: op(X)[i, k] = x[i * ld + k]; xt = 1: x[k * ld + i]
NmfOperand nmf_x_operand(const float* x, long long ld, long long bs, int xt) {
  return xt ? nmf_operand(x, 1, ld, bs) : nmf_operand(x, ld, 1, bs);
}

int nmf_x_check(const char* what, const float* x, long long ld, long long bs, int xt, int G, int rows, int cols) {
  HR_REQUIRE(xt == 0 || xt == 1, "%s: orientation flag %d: 0 (x[i * ld + k]) or 1 (x[k * ld + i])", what, xt);
  const long long row = xt ? rows : cols;      // length of a contiguous run
  HR_REQUIRE(ld >= row && ld <= (1LL << 40), "%s: leading dimension %lld: needs at least %lld (and at most 2^40)", what, ld, row);
  HR_REQUIRE(bs >= 0 && bs <= (1LL << 40) && (G == 1 || bs > 0), "%s: batch stride %lld with %d matrices: needs a positive "
             "stride (at most 2^40)", what, bs, G);
  HR_REQUIRE(x, "%s: null feature pointer", what);
  return HR_OK;
}

int nmf_launch(const char* what, bool update, NmfGemm& g, int G, hr_stream_t stream) {
  HR_REQUIRE((long long)G * g.splits <= kMaxG, "%s: %d matrices (times %d splits): at most %d", what, G, g.splits, kMaxG);
  // the tile is a function of the shape alone, so a shape always takes the same kernel and sums in the same order
  const long long large = (long long)((g.M + kTile - 1) / kTile) * ((g.N + kTile - 1) / kTile) * G * g.splits;
  const int tile = large < kFillGrid ? kSmallTile : kTile;
  const long long tiles_m = (g.M + tile - 1) / tile, tiles_n = (g.N + tile - 1) / tile;
  HR_REQUIRE(tiles_m * tiles_n <= 0x7fffffffLL, "%s: %lld tiles: too many", what, tiles_m * tiles_n);
  g.tiles_n = (int)tiles_n;
  const dim3 grid((unsigned)(tiles_m * tiles_n), (unsigned)(G * g.splits));
  if (update && tile == kTile) nmf_gemm_kernel<true, kTile><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  else if (update) nmf_gemm_kernel<true, kSmallTile><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  else if (tile == kTile) nmf_gemm_kernel<false, kTile><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  else nmf_gemm_kernel<false, kSmallTile><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  return hr_check_launch(what);
}

bool nmf_dims(int G, int a, int b, int c) {
  return G >= 1 && G <= kMaxG && a >= 1 && a <= kMaxDim && b >= 1 && b <= kMaxDim && c >= 1 && c <= kMaxDim;
}

// parts of the reduction over K for G Gram matrices of R columns, and the length of one part (a multiple of kBK)
void nmf_gram_split(int G, int K, int R, int* splits, int* kchunk) {
  const long long tr = (R + kTile - 1) / kTile, tiles = tr * tr * G;
  long long s = kGramTiles / tiles;
  const long long smax = (K + kGramMinK - 1) / kGramMinK;
  if (s > smax) s = smax;
  if (s > kMaxG / G) s = kMaxG / G;
  if (s < 1) s = 1;
  long long chunk = (K + s - 1) / s;
  chunk = (chunk + kBK - 1) / kBK * kBK;
  *kchunk = (int)chunk;
  *splits = (int)((K + chunk - 1) / chunk);
}

}  // namespace

extern "C" int hrnet_nmf_supported(int op, int a, int b) {
  switch (op) {
    case HR_NMF_UPDATE:
    case HR_NMF_GRAM:
    case HR_NMF_PRODUCT: return a >= 1 && a <= kMaxDim && b >= 1 && b <= kMaxDim;
    default: return 0;
  }
}

extern "C" int hrnet_nmf_update(const float* T, const float* F, const float* x, long long ldx, long long bsx, int xt,
                                const float* Gm, float* Tout, int G, int M, int K, int R, float eps, hr_stream_t stream) {
  HR_REQUIRE(hrnet_nmf_supported(HR_NMF_UPDATE, K, R) && nmf_dims(G, M, K, R), "nmf_update: G = %d, M = %d, K = %d, R = %d: "
             "needs 1 <= G <= %d and 1 <= M, K, R <= %d", G, M, K, R, kMaxG, kMaxDim);
  HR_REQUIRE(eps > 0.f, "nmf_update: eps = %g: must be positive", (double)eps);
  if (const int rc = nmf_x_check("nmf_update", x, ldx, bsx, xt, G, M, K)) return rc;
  HR_REQUIRE(T && F && Gm && Tout, "nmf_update: null pointer (T = %p, F = %p, Gm = %p, Tout = %p)", (const void*)T,
             (const void*)F, (const void*)Gm, (void*)Tout);
  HR_REQUIRE(Tout != T && Tout != F && Tout != Gm && Tout != x, "nmf_update: Tout aliases an input (the update is out of "
             "place: a tile's T Gm reads whole rows of T)");
  NmfGemm g = {};
  g.a1 = nmf_x_operand(x, ldx, bsx, xt);
  g.b1 = nmf_operand(F, 1, R, (long long)K * R);
  g.a2 = nmf_operand(T, R, 1, (long long)M * R);
  g.b2 = nmf_operand(Gm, 1, R, (long long)R * R);
  g.t = T; g.c = Tout; g.c_sm = R; g.c_bs = (long long)M * R; g.c_ss = 0;
  g.M = M; g.N = R; g.K1 = K; g.K2 = R; g.splits = 1; g.kchunk = (K + kBK - 1) / kBK * kBK; g.eps = eps;
  return nmf_launch("nmf_update", true, g, G, stream);
}

extern "C" int hrnet_nmf_gram_scratch(int G, int K, int R) {
  if (!hrnet_nmf_supported(HR_NMF_GRAM, K, R) || G < 1 || G > kMaxG) return 0;
  int splits, kchunk;
  nmf_gram_split(G, K, R, &splits, &kchunk);
  const long long floats = splits > 1 ? (long long)G * splits * R * R : 0;
  return floats <= 0x7fffffffLL ? (int)floats : 0;
}

extern "C" int hrnet_nmf_gram(const float* A, float* Gm, float* scratch, long long scratch_floats, int G, int K, int R,
                              hr_stream_t stream) {
  HR_REQUIRE(hrnet_nmf_supported(HR_NMF_GRAM, K, R) && nmf_dims(G, K, R, R), "nmf_gram: G = %d, K = %d, R = %d: needs "
             "1 <= G <= %d and 1 <= K, R <= %d", G, K, R, kMaxG, kMaxDim);
  HR_REQUIRE(A && Gm, "nmf_gram: null pointer (A = %p, Gm = %p)", (const void*)A, (void*)Gm);
  HR_REQUIRE((const void*)A != (const void*)Gm, "nmf_gram: Gm aliases A");
  int splits, kchunk;
  nmf_gram_split(G, K, R, &splits, &kchunk);
  const long long rr = (long long)R * R, need = splits > 1 ? (long long)G * splits * rr : 0;
  HR_REQUIRE(need <= 0x7fffffffLL, "nmf_gram: G = %d, K = %d, R = %d: the %d parts take %lld floats of scratch, more than "
             "2^31 - 1", G, K, R, splits, need);
  HR_REQUIRE(need == 0 || (scratch && scratch_floats >= need), "nmf_gram: scratch of %lld floats at %p: %lld are needed "
             "(hrnet_nmf_gram_scratch)", scratch_floats, (void*)scratch, need);
  HR_REQUIRE(need == 0 || (scratch != Gm && scratch != A), "nmf_gram: scratch aliases A or Gm");
  NmfGemm g = {};
  g.a1 = nmf_operand(A, 1, R, (long long)K * R);       // A^T: (R, K), element (i, k) = A[k * R + i]
  g.b1 = nmf_operand(A, 1, R, (long long)K * R);
  g.M = R; g.N = R; g.K1 = K; g.K2 = 0; g.splits = splits; g.kchunk = kchunk; g.c_sm = R;
  if (splits > 1) { g.c = scratch; g.c_bs = splits * rr; g.c_ss = rr; }
  else { g.c = Gm; g.c_bs = rr; g.c_ss = 0; }
  if (const int rc = nmf_launch("nmf_gram", false, g, G, stream)) return rc;
  if (splits == 1) return HR_OK;
  const long long total = (long long)G * rr, blocks = (total + 255) / 256;
  nmf_gram_reduce_kernel<<<(unsigned)(blocks < (1 << 16) ? blocks : (1 << 16)), 256, 0, (hipStream_t)stream>>>(
      scratch, Gm, rr, splits, total);
  return hr_check_launch("nmf_gram (reduce)");
}

extern "C" int hrnet_nmf_product(const float* x, long long ldx, long long bsx, int xt, const float* F, float* out, int G,
                                 int M, int K, int R, hr_stream_t stream) {
  HR_REQUIRE(hrnet_nmf_supported(HR_NMF_PRODUCT, K, R) && nmf_dims(G, M, K, R), "nmf_product: G = %d, M = %d, K = %d, R = %d: "
             "needs 1 <= G <= %d and 1 <= M, K, R <= %d", G, M, K, R, kMaxG, kMaxDim);
  if (const int rc = nmf_x_check("nmf_product", x, ldx, bsx, xt, G, M, K)) return rc;
  HR_REQUIRE(F && out, "nmf_product: null pointer (F = %p, out = %p)", (const void*)F, (void*)out);
  HR_REQUIRE(out != F && out != x, "nmf_product: out aliases an input");
  NmfGemm g = {};
  g.a1 = nmf_x_operand(x, ldx, bsx, xt);
  g.b1 = nmf_operand(F, 1, R, (long long)K * R);
  g.c = out; g.c_sm = R; g.c_bs = (long long)M * R;
  g.M = M; g.N = R; g.K1 = K; g.K2 = 0; g.splits = 1; g.kchunk = (K + kBK - 1) / kBK * kBK;
  return nmf_launch("nmf_product", false, g, G, stream);
}

extern "C" int hrnet_nmf_reconstruct(const float* Bs, const float* Cf, float* out, long long ldo, long long bso, int ot,
                                     int G, int D, int N, int R, hr_stream_t stream) {
  HR_REQUIRE(hrnet_nmf_supported(HR_NMF_PRODUCT, R, N) && nmf_dims(G, D, N, R), "nmf_reconstruct: G = %d, D = %d, N = %d, "
             "R = %d: needs 1 <= G <= %d and 1 <= D, N, R <= %d", G, D, N, R, kMaxG, kMaxDim);
  if (const int rc = nmf_x_check("nmf_reconstruct", out, ldo, bso, ot, G, D, N)) return rc;
  HR_REQUIRE(Bs && Cf, "nmf_reconstruct: null pointer (Bs = %p, Cf = %p)", (const void*)Bs, (const void*)Cf);
  HR_REQUIRE(out != Bs && out != Cf, "nmf_reconstruct: out aliases an input");
  NmfGemm g = {};
  const NmfOperand bases = nmf_operand(Bs, R, 1, (long long)D * R), coef = nmf_operand(Cf, R, 1, (long long)N * R);
  if (ot == 0) {         // out[d * ld + n]: rows d, columns n
    g.a1 = bases; g.b1 = coef; g.M = D; g.N = N;
  } else {               // out[n * ld + d]: the transposed product, rows n, columns d
    g.a1 = coef; g.b1 = bases; g.M = N; g.N = D;
  }
  g.c = out; g.c_sm = ldo; g.c_bs = bso;
  g.K1 = R; g.K2 = 0; g.splits = 1; g.kchunk = (R + kBK - 1) / kBK * kBK;
  return nmf_launch("nmf_reconstruct", false, g, G, stream);
}
