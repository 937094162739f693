// Cross-view heat-map fusion of multiview_pose_hrnet (reference lib/models/multiview_pose_hrnet.py:57-71): every view's
// heat maps are corrected by the other views' maps through one Linear(P, P, bias=False) per ordered view pair.
//
//   forward   F[b,i,k,:] = w_self * H[b,i,k,:] + w_other * sum_{j != i} H[b,j,k,:] @ W[n(i,j)]^T
//   dH        dH[b,j,k,:] = w_self * dF[b,j,k,:] + w_other * sum_{i != j} dF[b,i,k,:] @ W[n(i,j)]
//   dW        dW[n(i,j)] = w_other * dF[:,i]^T @ H[:,j]                       (summed over the M = B * K rows)
//   n(i,j) = i * (V - 1) + (rank of j among the views other than i)
//
// H, F, dF, dH are [B][V][K][P] f32; W[n] is the module's own [P_out][P_in] tensor, read in place through a table of
// V * (V - 1) pointers passed by value: nothing is packed, transposed or copied.
//
// This is a skinny GEMM: M rows against V * (V - 1) * P * P weights (805 MB at V = 4, P = 4096), so the weights are the
// traffic and every kernel is organised around touching each weight element once. All products run on
// mfma_f32_16x16x4f32 (A: lane (i = l & 15, g = l >> 4) holds A[i][g], B: lane (j, g) holds B[g][j], D: column = l & 15,
// row = 4 * (l >> 4) + register). The k order inside a step is free as long as A and B agree, so both operands are
// loaded as 16-byte (dH: 8-byte for W) vectors and component c of the vector is k-step c.
//
//   forward   workgroup = 4 waves, one block of 32 output positions of one target view, MT tiles of 16 rows. The waves
//             split the reduction ((V - 1) sources x 64-position chunks, chunk c goes to wave c % 4); a wave keeps its
//             32 x 64 weight tile in registers and walks ALL M tiles against it (H is small and comes from L2), so a
//             weight element is read once for M <= 16 * 12 = 192. The four partial sums meet in LDS and are added in wave
//             order: no atomics, one fixed order. Rows of W = A rows, rows of H = B columns, so a lane ends up with four
//             consecutive output positions of one row: 16-byte stores.
//   dH        the same structure with the roles of the weight axes swapped: a workgroup owns 32 positions p of one source
//             view, the reduction runs over (V - 1) targets x 64-row chunks of W, dF rows = A rows, W = B with 8-byte
//             loads (lane j holds positions 2j, 2j + 1: 128 contiguous bytes per weight row).
//   dW        one wave per 64 x 64 tile of one pair: 16 accumulators, K = M rows in steps of 4, each element of dW written
//             once, w_other folded into the store. No split, so no scratch and nothing to reduce.
// Tails: rows >= M and positions >= P are loaded as zeros (never dereferenced) and not stored, so every MFMA runs with
// all 64 lanes on; M is padded in registers only. The vector paths need P % 4 == 0 and 16-byte aligned pointers;
// anything else (rows of W are then not 16-byte aligned) takes the element-wise loads of the same kernels.
#include "common.h"

namespace {

constexpr int kMaxV = 4;
constexpr int kMaxPairs = kMaxV * (kMaxV - 1);
constexpr int kWaves = 4;              // waves of a forward / dH workgroup: the split of the reduction
constexpr int kBlk = 32;               // output positions of a forward / dH workgroup
constexpr int kChunk = 64;             // reduction positions of one step of a wave
constexpr int kMaxMT = 12;             // 16-row M tiles held against one weight tile
constexpr int kDwTile = 64;
constexpr int kMaxP = 1 << 20;
constexpr long long kMaxElems = (1LL << 31) - 1;

struct VfSrc { const float* w[kMaxPairs]; };
struct VfDst { float* w[kMaxPairs]; };

#define VF_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// row[p .. p + 3], zeros beyond P
template <bool VEC>
__device__ __forceinline__ f32x4 vf_ld4(const float* __restrict__ row, int p, int P) {
  if (VEC) return p < P ? *(const f32x4*)(row + p) : f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 v;
  v.x = p < P ? row[p] : 0.f;
  v.y = p + 1 < P ? row[p + 1] : 0.f;
  v.z = p + 2 < P ? row[p + 2] : 0.f;
  v.w = p + 3 < P ? row[p + 3] : 0.f;
  return v;
}

template <bool VEC>
__device__ __forceinline__ f32x2 vf_ld2(const float* __restrict__ row, int p, int P) {
  if (VEC) return p < P ? *(const f32x2*)(row + p) : f32x2{0.f, 0.f};
  f32x2 v;
  v.x = p < P ? row[p] : 0.f;
  v.y = p + 1 < P ? row[p + 1] : 0.f;
  return v;
}

// element offset of row m = b * K + k of view 0 in a [B][V][K][P] tensor
__device__ __forceinline__ int vf_row(int m, int V, int K, int P) {
  const int b = m / K;
  return ((b * V) * K + (m - b * K)) * P;
}

// the four waves' partial tiles of one pass meet in LDS; wave w then owns tiles w, w + 4, ... and adds the partials in
// wave order
template <int MT>
__device__ __forceinline__ void vf_reduce(f32x4 (*red)[MT][64], const f32x4* acc, int wave, int lane,
                                          f32x4* out) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) red[wave][mt][lane] = acc[mt];
  __syncthreads();
#pragma unroll
  for (int it = 0; it < (MT + kWaves - 1) / kWaves; ++it) {
    const int mt = wave + kWaves * it;
    if (mt < MT) {
      f32x4 s = red[0][mt][lane];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) s += red[w][mt][lane];
      out[it] = s;
    }
  }
  __syncthreads();
}

// grid (ceil(P / 32), V, ceil(mtiles / MT)), 256 threads. UN = weight chunks a wave has in flight.
template <int MT, int UN, bool VEC>
__global__ __launch_bounds__(64 * kWaves) void vf_fwd_kernel(const float* __restrict__ H, const VfSrc W,
                                                             float* __restrict__ F, int M, int V, int K, int P,
                                                             float w_self, float w_other) {
  constexpr int OT = kBlk / 16, NIT = (MT + kWaves - 1) / kWaves;
  __shared__ f32x4 red[kWaves][MT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int i = blockIdx.y, o0 = blockIdx.x * kBlk, m0 = blockIdx.z * (16 * MT);
  const long long view = (long long)K * P;
  int hoff[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + mt * 16 + j;
    hoff[mt] = m < M ? vf_row(m, V, K, P) : -1;
  }
  f32x4 acc[OT][MT];
#pragma unroll
  for (int ot = 0; ot < OT; ++ot)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[ot][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nchunk = (P + kChunk - 1) / kChunk, total = (V - 1) * nchunk;
  for (int c0 = wave; c0 < total; c0 += kWaves * UN) {
    f32x4 w[UN][OT][4];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int c = c0 + u * kWaves;
      const int jj = c < total ? c / nchunk : 0, pc = (c - jj * nchunk) * kChunk;
      const float* __restrict__ Wn = W.w[i * (V - 1) + jj];
#pragma unroll
      for (int ot = 0; ot < OT; ++ot) {
        const int o = o0 + ot * 16 + j;
#pragma unroll
        for (int t = 0; t < 4; ++t)
          w[u][ot][t] = (c < total && o < P) ? vf_ld4<VEC>(Wn + (long long)o * P, pc + 16 * t + 4 * g, P)
                                             : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int c = c0 + u * kWaves;
      if (c >= total) break;
      const int jj = c / nchunk, pc = (c - jj * nchunk) * kChunk;
      const float* __restrict__ Hj = H + (jj < i ? jj : jj + 1) * view;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        f32x4 h[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
          h[t] = hoff[mt] >= 0 ? vf_ld4<VEC>(Hj + hoff[mt], pc + 16 * t + 4 * g, P) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int ot = 0; ot < OT; ++ot) acc[ot][mt] = VF_MFMA(w[u][ot][t][e], h[t][e], acc[ot][mt]);
      }
    }
  }
#pragma unroll
  for (int ot = 0; ot < OT; ++ot) {
    f32x4 s[NIT];
    vf_reduce<MT>(red, acc[ot], wave, lane, s);
    const int o = o0 + ot * 16 + 4 * g;          // D row 4g + r = output position o + r, D column j = row m
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int mt = wave + kWaves * it, m = m0 + mt * 16 + j;
      if (mt >= MT || m >= M || o >= P) continue;
      const long long off = i * view + vf_row(m, V, K, P);
      const f32x4 hs = vf_ld4<VEC>(H + off, o, P);
      const f32x4 v = w_self * hs + w_other * s[it];
      float* __restrict__ dst = F + off;
      if (VEC) {
        *(f32x4*)(dst + o) = v;
      } else {
        dst[o] = v.x;
        if (o + 1 < P) dst[o + 1] = v.y;
        if (o + 2 < P) dst[o + 2] = v.z;
        if (o + 3 < P) dst[o + 3] = v.w;
      }
    }
  }
}

// grid (ceil(P / 32), V, ceil(mtiles / MT)), 256 threads
template <int MT, int UN, bool VEC>
__global__ __launch_bounds__(64 * kWaves) void vf_dh_kernel(const float* __restrict__ dF, const VfSrc W,
                                                            float* __restrict__ dH, int M, int V, int K, int P,
                                                            float w_self, float w_other) {
  constexpr int NIT = (MT + kWaves - 1) / kWaves, NU = kChunk / 16;
  __shared__ f32x4 red[kWaves][MT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int jv = blockIdx.y, p = blockIdx.x * kBlk + 2 * j, m0 = blockIdx.z * (16 * MT);
  const long long view = (long long)K * P;
  int hoff[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + mt * 16 + j;
    hoff[mt] = m < M ? vf_row(m, V, K, P) : -1;
  }
  f32x4 acc[2][MT];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[q][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nchunk = (P + kChunk - 1) / kChunk, total = (V - 1) * nchunk;
  for (int c0 = wave; c0 < total; c0 += kWaves * UN) {
    f32x2 w[UN][NU][4];                            // k step (s, t): row o = oc + 16 s + 4 g + t of W
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int c = c0 + u * kWaves;
      const int ii = c < total ? c / nchunk : 0, oc = (c - ii * nchunk) * kChunk;
      const int iv = ii < jv ? ii : ii + 1;
      const float* __restrict__ Wn = W.w[iv * (V - 1) + (jv < iv ? jv : jv - 1)];
#pragma unroll
      for (int s = 0; s < NU; ++s)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int o = oc + 16 * s + 4 * g + t;
          w[u][s][t] = (c < total && o < P) ? vf_ld2<VEC>(Wn + (long long)o * P, p, P) : f32x2{0.f, 0.f};
        }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int c = c0 + u * kWaves;
      if (c >= total) break;
      const int ii = c / nchunk, oc = (c - ii * nchunk) * kChunk;
      const float* __restrict__ dFi = dF + (ii < jv ? ii : ii + 1) * view;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        f32x4 a[NU];
#pragma unroll
        for (int s = 0; s < NU; ++s)
          a[s] = hoff[mt] >= 0 ? vf_ld4<VEC>(dFi + hoff[mt], oc + 16 * s + 4 * g, P) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NU; ++s)
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int q = 0; q < 2; ++q) acc[q][mt] = VF_MFMA(a[s][t], w[u][s][t][q], acc[q][mt]);
      }
    }
  }
  f32x4 s0[NIT], s1[NIT];
  vf_reduce<MT>(red, acc[0], wave, lane, s0);
  vf_reduce<MT>(red, acc[1], wave, lane, s1);
  if (p >= P) return;                              // D column j = positions p, p + 1; D row 4g + r = row m + r
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int mt = wave + kWaves * it;
    if (mt >= MT) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + mt * 16 + 4 * g + r;
      if (m >= M) continue;
      const long long off = jv * view + vf_row(m, V, K, P);
      const f32x2 d = vf_ld2<VEC>(dF + off, p, P);
      const f32x2 v = {w_self * d.x + w_other * s0[it][r], w_self * d.y + w_other * s1[it][r]};
      float* __restrict__ dst = dH + off;
      if (VEC) {
        *(f32x2*)(dst + p) = v;
      } else {
        dst[p] = v.x;
        if (p + 1 < P) dst[p + 1] = v.y;
      }
    }
  }
}

// one wave: tile (64 rows o from 64 * blockIdx.y, 64 columns p from 64 * blockIdx.x) of listed pair blockIdx.z
template <bool VEC>
__global__ __launch_bounds__(64) void vf_dw_kernel(const float* __restrict__ H, const float* __restrict__ dF,
                                                   const VfDst dW, int M, int V, int K, int P, float w_other) {
  const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
  const int n = blockIdx.z;
  float* __restrict__ out = dW.w[n];
  if (!out) return;                                // the whole wave
  const int i = n / (V - 1), jj = n - i * (V - 1), jv = jj < i ? jj : jj + 1;
  const int o = blockIdx.y * kDwTile + 4 * j, p = blockIdx.x * kDwTile + 4 * j;
  const long long view = (long long)K * P;
  const float* __restrict__ dFi = dF + i * view;
  const float* __restrict__ Hj = H + jv * view;
  f32x4 acc[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int q2 = 0; q2 < 4; ++q2) acc[q][q2] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int ms = 0; ms < M; ms += 4) {
    const int m = ms + g;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (m < M) {
      const int off = vf_row(m, V, K, P);
      a = vf_ld4<VEC>(dFi + off, o, P);            // A row j of group q = position o + q
      b = vf_ld4<VEC>(Hj + off, p, P);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int q2 = 0; q2 < 4; ++q2) acc[q][q2] = VF_MFMA(a[q], b[q2], acc[q][q2]);
  }
  if (p >= P) return;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = blockIdx.y * kDwTile + 4 * (4 * g + r) + q;   // D row 4g + r of group q
      if (orow >= P) continue;
      const f32x4 v = {w_other * acc[q][0][r], w_other * acc[q][1][r], w_other * acc[q][2][r], w_other * acc[q][3][r]};
      float* __restrict__ dst = out + (long long)orow * P;
      if (VEC) {
        *(f32x4*)(dst + p) = v;
      } else {
        dst[p] = v.x;
        if (p + 1 < P) dst[p + 1] = v.y;
        if (p + 2 < P) dst[p + 2] = v.z;
        if (p + 3 < P) dst[p + 3] = v.w;
      }
    }
}

bool vf_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

int vf_mt(int M) {
  const int mtiles = (M + 15) / 16, mt = 2 * ((mtiles + 1) / 2);
  return mt > kMaxMT ? kMaxMT : mt;
}

int vf_shape(const char* what, int dtype, int B, int V, int K, int P) {
  HR_REQUIRE(hrnet_view_fusion_supported(dtype, V, P), "%s: dtype = %d, V = %d, P = %d: needs f32 (HR_F32 = 0), "
             "2 <= V <= %d and 1 <= P <= %d", what, dtype, V, P, kMaxV, kMaxP);
  HR_REQUIRE(B >= 1 && K >= 1, "%s: B = %d, K = %d: both must be at least 1", what, B, K);
  HR_REQUIRE((long long)B * V * K <= kMaxElems / P, "%s: B * V * K * P = %lld elements, more than 2^31 - 1 (B = %d, "
             "V = %d, K = %d, P = %d)", what, (long long)B * V * K * P, B, V, K, P);
  HR_REQUIRE(((long long)B * K + 16 * kMaxMT - 1) / (16 * kMaxMT) <= 65535, "%s: B * K = %lld rows: too many", what,
             (long long)B * K);
  return HR_OK;
}

template <bool VEC, bool DH>
void vf_launch(const float* X, const VfSrc& W, float* Y, int M, int V, int K, int P, float w_self, float w_other,
               hipStream_t s) {
  const int MT = vf_mt(M);
  const dim3 grid((unsigned)((P + kBlk - 1) / kBlk), (unsigned)V, (unsigned)(((M + 15) / 16 + MT - 1) / MT));
#define VF_CASE(mt, un)                                                                              \
  case mt:                                                                                           \
    if (DH)                                                                                          \
      vf_dh_kernel<mt, un, VEC><<<grid, 64 * kWaves, 0, s>>>(X, W, Y, M, V, K, P, w_self, w_other);  \
    else                                                                                             \
      vf_fwd_kernel<mt, un, VEC><<<grid, 64 * kWaves, 0, s>>>(X, W, Y, M, V, K, P, w_self, w_other); \
    break;
  switch (MT) {
    VF_CASE(2, 2)
    VF_CASE(4, 2)
    VF_CASE(6, 1)
    VF_CASE(8, 1)
    VF_CASE(10, 1)
    default:
    VF_CASE(12, 1)
  }
#undef VF_CASE
}

}  // namespace

extern "C" int hrnet_view_fusion_supported(int dtype, int V, int P) {
  return dtype == HR_F32 && V >= 2 && V <= kMaxV && P >= 1 && P <= kMaxP;
}

extern "C" int hrnet_view_fusion(int dtype, const float* H, const void* const* W, float* F, int B, int V, int K, int P,
                                 float w_self, float w_other, hr_stream_t stream) {
  if (const int rc = vf_shape("view_fusion", dtype, B, V, K, P)) return rc;
  HR_REQUIRE(H && W && F, "view_fusion: null pointer (H = %p, W = %p, F = %p)", (const void*)H, (const void*)W, (void*)F);
  HR_REQUIRE((const void*)H != (const void*)F, "view_fusion: F aliases H");
  VfSrc src = {};
  bool vec = P % 4 == 0 && vf_aligned(H) && vf_aligned(F);
  for (int n = 0; n < V * (V - 1); ++n) {
    HR_REQUIRE(W[n], "view_fusion: W[%d] is null", n);
    src.w[n] = (const float*)W[n];
    vec = vec && vf_aligned(W[n]);
  }
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    vf_launch<true, false>(H, src, F, B * K, V, K, P, w_self, w_other, s);
  else
    vf_launch<false, false>(H, src, F, B * K, V, K, P, w_self, w_other, s);
  return hr_check_launch("view_fusion");
}

extern "C" int hrnet_view_fusion_bwd(int dtype, const float* H, const void* const* W, const float* dF, float* dH,
                                     void* const* dW, int B, int V, int K, int P, float w_self, float w_other,
                                     hr_stream_t stream) {
  if (const int rc = vf_shape("view_fusion_bwd", dtype, B, V, K, P)) return rc;
  HR_REQUIRE(dF, "view_fusion_bwd: dF is null");
  HR_REQUIRE(dH || dW, "view_fusion_bwd: dH and dW are both null: nothing to compute");
  hipStream_t s = (hipStream_t)stream;
  const int M = B * K, pairs = V * (V - 1);
  if (dH) {
    HR_REQUIRE(W, "view_fusion_bwd: W is null with dH asked for");
    HR_REQUIRE((const void*)dH != (const void*)dF, "view_fusion_bwd: dH aliases dF");
    VfSrc src = {};
    bool vec = P % 4 == 0 && vf_aligned(dF) && vf_aligned(dH);
    for (int n = 0; n < pairs; ++n) {
      HR_REQUIRE(W[n], "view_fusion_bwd: W[%d] is null", n);
      src.w[n] = (const float*)W[n];
      vec = vec && vf_aligned(W[n]);
    }
    if (vec)
      vf_launch<true, true>(dF, src, dH, M, V, K, P, w_self, w_other, s);
    else
      vf_launch<false, true>(dF, src, dH, M, V, K, P, w_self, w_other, s);
  }
  if (dW) {
    HR_REQUIRE(H, "view_fusion_bwd: H is null with dW asked for");
    VfDst dst = {};
    bool vec = P % 4 == 0 && vf_aligned(dF) && vf_aligned(H), any = false;
    for (int n = 0; n < pairs; ++n) {
      dst.w[n] = (float*)dW[n];
      if (dW[n]) {
        any = true;
        vec = vec && vf_aligned(dW[n]);
        HR_REQUIRE(dW[n] != (const void*)dF && dW[n] != (const void*)H, "view_fusion_bwd: dW[%d] aliases dF or H", n);
      }
    }
    if (any) {
      const unsigned tiles = (unsigned)((P + kDwTile - 1) / kDwTile);
      const dim3 grid(tiles, tiles, (unsigned)pairs);
      if (vec)
        vf_dw_kernel<true><<<grid, 64, 0, s>>>(H, dF, dst, M, V, K, P, w_other);
      else
        vf_dw_kernel<false><<<grid, 64, 0, s>>>(H, dF, dst, M, V, K, P, w_other);
    }
  }
  return hr_check_launch("view_fusion_bwd");
}
