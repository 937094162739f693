// Transformer kernels of pose_hrnet_transformer, the reference's PoseFormer head (reference
// lib/models/pose_hrnet_transformer.py:21-85 Mlp / Attention / Block, :195-221 the two encoders): LayerNorm, a dense
// linear layer, attention on a packed qkv, the weighted mean over frames and the broadcast add of a position embedding,
// each forward and backward. Everything is f32 on row-major (rows, C) tensors with 64-bit element offsets; nn.Linear
// weights (out, in) are read in place - nothing is packed, transposed or cached.
//
// The head is 58 MB of weights against 36 .. 756 rows: every product is a skinny GEMM and the launch boundaries, not the
// bytes or the flops, are what a step pays for (DESIGN, PoseFormer section). The kernels are therefore plain: one fixed
// tiling per product, no tuning tables.
//
// No float atomics anywhere: every sum has one fixed order, so a call is bit-reproducible.
//
//   layernorm      one wave per row: mean, then the centred second moment (two passes over a row that sits in L1/L2),
//                  rstd = 1 / sqrt(var + eps); the row sums are f64 (see tf_row_stats).
//   layernorm_bwd  dx: one wave per row, statistics recomputed from x; the row's (mean, rstd) go to scratch. dgamma / dbeta:
//                  two stages - (64 columns x 64 rows) partial column sums, then the parts added in order.
//   linear         y = [res +] rowscale[row] * act(x W^T + b) on mfma_f32_16x16x4f32 (A: lane (i = l & 15, g = l >> 4)
//                  holds A[i][g], B: lane (j, g) holds B[g][j], D: column = l & 15, row = 4 * (l >> 4) + register). A
//                  workgroup of 4 waves owns 16 outputs x 64 rows; the waves split the reduction (chunks of 16 inputs,
//                  chunk c goes to wave c % 4), the partial tiles meet in LDS and are added in wave order. Rows of W = A
//                  rows, rows of x = B columns, so a lane ends with 4 consecutive outputs of one row. With act = GELU the
//                  pre-activation is also stored (`pre`), and the backward TAKES it as an input rather than recomputing
//                  the product.
//   linear_bwd     g = dy * rowscale[row] * act'(pre) is formed in the loads of both kernels, never stored.
//                  dx = g W: 64 input columns x 64 rows per workgroup, the 4 waves split the reduction over the outputs.
//                  dW = g^T x and db = column sums of g: one wave per 64 x 64 tile of dW, K = rows in steps of 4; the
//                  tiles of the first column block also sum db (runs of 16 steps per lane, then the lanes in a fixed shuffle
//                  order).
//   attention      one wave per (sequence, head), lane n = query n (N <= 64). Scores and probabilities live in LDS
//                  ([key][query], 16 KB); k and v rows are wave-uniform reads. Backward recomputes the probabilities
//                  from qkv, keeps dS in a second LDS tile and returns dq (lane = query), dk and dv (lane = key).
//   frame_mean     out[s, :] = sum_f w[f] x[s, f, :] + b (the reference's Conv1d(F -> 1, kernel 1), :187, :219). Backward:
//                  dx elementwise; dw[f] and db are one workgroup each, a strided f64 sum then a fixed LDS tree.
//   add_rows       y[r, :] = x[r, :] + pos[r % period, :] (the position embeddings, :200, :212). Its backward is a
//                  pass-through for x and frame_mean with unit weights for pos.
// Tails: rows and columns beyond the tensor are loaded as zeros (never dereferenced) and not stored. The 16-byte paths
// need the inner extents to be multiples of 4 and 16-byte aligned pointers; anything else (Cin = 2, Cout = 42) takes the
// element-wise loads of the same kernels.
#include "common.h"

namespace {

constexpr int kWaves = 4;
constexpr int kMT = 4;                 // 16-row tiles of a linear / dx workgroup: 64 rows
constexpr int kMaxC = 1 << 16;         // widest row
constexpr long long kMaxRows = 1LL << 22;
constexpr int kMaxN = 64, kMaxHd = 128;
constexpr int kSStride = 65;           // LDS row stride of the [key][query] tiles: both access directions conflict-free
constexpr int kLnRows = 64;            // rows of one partial column sum of layernorm_bwd

#define TF_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ float tf_gelu(float z) { return 0.5f * z * (1.f + erff(z * 0.70710678118654752440f)); }
__device__ __forceinline__ float tf_gelu_grad(float z) {
  return 0.5f * (1.f + erff(z * 0.70710678118654752440f)) + z * 0.39894228040143267794f * expf(-0.5f * z * z);
}

// row[p .. p + 3], zeros beyond P
template <bool VEC>
__device__ __forceinline__ f32x4 tf_ld4(const float* __restrict__ row, int p, int P) {
  if (VEC) return p < P ? *(const f32x4*)(row + p) : f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 v;
  v.x = p < P ? row[p] : 0.f;
  v.y = p + 1 < P ? row[p + 1] : 0.f;
  v.z = p + 2 < P ? row[p + 2] : 0.f;
  v.w = p + 3 < P ? row[p + 3] : 0.f;
  return v;
}

template <bool VEC>
__device__ __forceinline__ void tf_st4(float* __restrict__ row, int p, int P, f32x4 v) {
  if (p >= P) return;
  if (VEC) {
    *(f32x4*)(row + p) = v;
    return;
  }
  row[p] = v.x;
  if (p + 1 < P) row[p + 1] = v.y;
  if (p + 2 < P) row[p + 2] = v.z;
  if (p + 3 < P) row[p + 3] = v.w;
}

// g[row][o .. o + 3] = dy * rowscale[row] * act'(pre), zeros beyond Cout
template <bool VEC, bool GELU>
__device__ __forceinline__ f32x4 tf_ldg4(const float* __restrict__ dy, const float* __restrict__ pre, float rs,
                                         long long off, int o, int Cout) {
  f32x4 g = tf_ld4<VEC>(dy + off, o, Cout);
  if (GELU) {
    const f32x4 z = tf_ld4<VEC>(pre + off, o, Cout);
    g.x *= tf_gelu_grad(z.x);
    g.y *= tf_gelu_grad(z.y);
    g.z *= tf_gelu_grad(z.z);
    g.w *= tf_gelu_grad(z.w);
  }
  return g * rs;
}

// the four waves' partial tiles meet in LDS; wave w then owns row tile w and adds the partials in wave order
__device__ __forceinline__ f32x4 tf_reduce(f32x4 (*red)[kMT][64], const f32x4* acc, int wave, int lane) {
#pragma unroll
  for (int mt = 0; mt < kMT; ++mt) red[wave][mt][lane] = acc[mt];
  __syncthreads();
  f32x4 s = red[0][wave][lane];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) s += red[w][wave][lane];
  __syncthreads();
  return s;
}

// ---------------------------------------------------------------------------------------------------------- layernorm

__device__ __forceinline__ double tf_wave_sum64d(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// The row statistics and the backward's two row means are formed in f64: a row of dx sums to zero in exact arithmetic,
// and an f32 mean leaves a SYSTEMATIC residue in every element of the row (C times the mean's rounding), which the sums
// over rows that follow (a bias gradient upstream) would collect. The rows are short and few: the f64 rate is not felt.
__device__ __forceinline__ void tf_row_stats(const float* __restrict__ xr, int C, int lane, float eps, double& mean,
                                             double& rstd) {
  double s = 0.0;
  for (int c = lane; c < C; c += 64) s += (double)xr[c];
  mean = tf_wave_sum64d(s) / (double)C;
  double q = 0.0;
  for (int c = lane; c < C; c += 64) {
    const double d = (double)xr[c] - mean;
    q += d * d;
  }
  rstd = 1.0 / sqrt(tf_wave_sum64d(q) / (double)C + (double)eps);
}

// grid ceil(rows / 4), 256 threads: one wave per row
__global__ __launch_bounds__(256) void tf_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ y,
                                                        long long rows, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* __restrict__ xr = x + r * C;
  double mean, rstd;
  tf_row_stats(xr, C, lane, eps, mean, rstd);
  for (int c = lane; c < C; c += 64)
    y[r * C + c] = (float)(((double)xr[c] - mean) * rstd * (double)gamma[c] + (double)beta[c]);
}

// dx of one row per wave; stats[r] = (mean, rstd) for the column sums
__global__ __launch_bounds__(256) void tf_ln_dx_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ dy, float* __restrict__ dx,
                                                       float* __restrict__ stats, long long rows, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* __restrict__ xr = x + r * C;
  const float* __restrict__ dr = dy + r * C;
  double mean, rstd;
  tf_row_stats(xr, C, lane, eps, mean, rstd);
  if (stats && lane == 0) {
    stats[2 * r] = (float)mean;
    stats[2 * r + 1] = (float)rstd;
  }
  if (!dx) return;
  double s1 = 0.0, s2 = 0.0;
  for (int c = lane; c < C; c += 64) {
    const double gd = (double)dr[c] * (double)gamma[c];
    s1 += gd * (((double)xr[c] - mean) * rstd);
    s2 += gd;
  }
  s1 = tf_wave_sum64d(s1) / (double)C;
  s2 = tf_wave_sum64d(s2) / (double)C;
  for (int c = lane; c < C; c += 64) {
    const double xh = ((double)xr[c] - mean) * rstd;
    dx[r * C + c] = (float)(rstd * ((double)dr[c] * (double)gamma[c] - s2 - xh * s1));
  }
}

// grid (ceil(C / 64), parts), 64 threads: part[p][0][c] = sum dy * xhat, part[p][1][c] = sum dy over the part's rows
__global__ __launch_bounds__(64) void tf_ln_cols_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                        const float* __restrict__ stats, float* __restrict__ part,
                                                        long long rows, int C) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  const long long r0 = (long long)blockIdx.y * kLnRows, r1 = r0 + kLnRows < rows ? r0 + kLnRows : rows;
  float dg = 0.f, db = 0.f;
  for (long long r = r0; r < r1; ++r) {
    const float d = dy[r * C + c];
    dg += d * ((x[r * C + c] - stats[2 * r]) * stats[2 * r + 1]);
    db += d;
  }
  part[((long long)blockIdx.y * 2 + 0) * C + c] = dg;
  part[((long long)blockIdx.y * 2 + 1) * C + c] = db;
}

__global__ __launch_bounds__(64) void tf_ln_cols_sum_kernel(const float* __restrict__ part, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int parts, int C) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  float dg = 0.f, db = 0.f;
  for (int p = 0; p < parts; ++p) {
    dg += part[((long long)p * 2 + 0) * C + c];
    db += part[((long long)p * 2 + 1) * C + c];
  }
  if (dgamma) dgamma[c] = dg;
  if (dbeta) dbeta[c] = db;
}

// ------------------------------------------------------------------------------------------------------------- linear

// grid (ceil(Cout / 16), ceil(rows / 64)), 256 threads
template <bool VEC, bool GELU>
__global__ __launch_bounds__(64 * kWaves) void tf_linear_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                                const float* __restrict__ bias,
                                                                const float* __restrict__ res,
                                                                const float* __restrict__ rs, float* __restrict__ y,
                                                                float* __restrict__ pre, long long rows, int Cin,
                                                                int Cout) {
  __shared__ f32x4 red[kWaves][kMT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int o0 = blockIdx.x * 16;
  const long long m0 = (long long)blockIdx.y * (16 * kMT);
  const int ow = o0 + j;                                   // A row j: output o0 + j
  f32x4 acc[kMT];
#pragma unroll
  for (int mt = 0; mt < kMT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nchunk = (Cin + 15) / 16;
  for (int c = wave; c < nchunk; c += kWaves) {
    const int k = c * 16 + 4 * g;
    const f32x4 w = ow < Cout ? tf_ld4<VEC>(W + (long long)ow * Cin, k, Cin) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 h[kMT];
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) {
      const long long m = m0 + mt * 16 + j;
      h[mt] = m < rows ? tf_ld4<VEC>(x + m * Cin, k, Cin) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[mt] = TF_MFMA(w[e], h[mt][e], acc[mt]);
  }
  const f32x4 s = tf_reduce(red, acc, wave, lane);
  const long long m = m0 + wave * 16 + j;                  // D column j = row m, D row 4g + r = output o0 + 4g + r
  const int o = o0 + 4 * g;
  if (m >= rows || o >= Cout) return;
  f32x4 v = s;
  if (bias) v += tf_ld4<false>(bias, o, Cout);
  if (GELU) {
    if (pre) tf_st4<VEC>(pre + m * Cout, o, Cout, v);
    v = f32x4{tf_gelu(v.x), tf_gelu(v.y), tf_gelu(v.z), tf_gelu(v.w)};
  }
  if (rs) v *= rs[m];
  if (res) v += tf_ld4<VEC>(res + m * Cout, o, Cout);
  tf_st4<VEC>(y + m * Cout, o, Cout, v);
}

// dx = g W. grid (ceil(Cin / 64), ceil(rows / 64)), 256 threads; lane j holds input columns i0 + 4j .. + 3
template <bool VEC, bool GELU>
__global__ __launch_bounds__(64 * kWaves) void tf_linear_dx_kernel(const float* __restrict__ dy,
                                                                   const float* __restrict__ pre,
                                                                   const float* __restrict__ rs,
                                                                   const float* __restrict__ W, float* __restrict__ dx,
                                                                   long long rows, int Cin, int Cout) {
  __shared__ f32x4 red[kWaves][kMT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int p = blockIdx.x * 64 + 4 * j;
  const long long m0 = (long long)blockIdx.y * (16 * kMT);
  float scale[kMT];
#pragma unroll
  for (int mt = 0; mt < kMT; ++mt) {
    const long long m = m0 + mt * 16 + j;
    scale[mt] = m < rows ? (rs ? rs[m] : 1.f) : 0.f;
  }
  f32x4 acc[4][kMT];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) acc[q][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nchunk = (Cout + 15) / 16;
  for (int c = wave; c < nchunk; c += kWaves) {
    const int o = c * 16 + 4 * g;                          // k step t: output o + t
    f32x4 w[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      w[t] = o + t < Cout ? tf_ld4<VEC>(W + (long long)(o + t) * Cin, p, Cin) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) {
      const long long m = m0 + mt * 16 + j;
      const f32x4 a = m < rows ? tf_ldg4<VEC, GELU>(dy, pre, scale[mt], m * Cout, o, Cout) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q][mt] = TF_MFMA(a[t], w[t][q], acc[q][mt]);
    }
  }
  f32x4 s[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) s[q] = tf_reduce(red, acc[q], wave, lane);
  if (p >= Cin) return;                                    // D column j = columns p + q, D row 4g + r = row m + r
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long m = m0 + wave * 16 + 4 * g + r;
    if (m >= rows) continue;
    tf_st4<VEC>(dx + m * Cin, p, Cin, f32x4{s[0][r], s[1][r], s[2][r], s[3][r]});
  }
}

// dW = g^T x, db = column sums of g. One wave: tile (64 outputs from 64 * blockIdx.y, 64 inputs from 64 * blockIdx.x)
template <bool VEC, bool GELU>
__global__ __launch_bounds__(64) void tf_linear_dw_kernel(const float* __restrict__ dy, const float* __restrict__ pre,
                                                          const float* __restrict__ rs, const float* __restrict__ x,
                                                          float* __restrict__ dW, float* __restrict__ db, long long rows,
                                                          int Cin, int Cout) {
  const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
  const int o = blockIdx.y * 64 + 4 * j, p = blockIdx.x * 64 + 4 * j;
  const bool do_w = dW != nullptr, do_b = db != nullptr && blockIdx.x == 0;
  f32x4 acc[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int q2 = 0; q2 < 4; ++q2) acc[q][q2] = f32x4{0.f, 0.f, 0.f, 0.f};
  // db: a lane's rows are summed in runs of 16 steps, the runs then added: two short sums rather than one long one
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f}, brun = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (long long ms = 0; ms < rows; ms += 4) {
    const long long m = ms + g;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (m < rows) {
      a = tf_ldg4<VEC, GELU>(dy, pre, rs ? rs[m] : 1.f, m * Cout, o, Cout);   // A row j of group q = output o + q
      if (do_w) b = tf_ld4<VEC>(x + m * Cin, p, Cin);
    }
    brun += a;
    if ((ms & 63) == 60) {
      bsum += brun;
      brun = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (do_w) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int q2 = 0; q2 < 4; ++q2) acc[q][q2] = TF_MFMA(a[q], b[q2], acc[q][q2]);
    }
  }
  bsum += brun;
  if (do_b) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = bsum[e];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (g == 0 && o + e < Cout) db[o + e] = v;
    }
  }
  if (!do_w || p >= Cin) return;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = blockIdx.y * 64 + 4 * (4 * g + r) + q;   // D row 4g + r of group q
      if (orow >= Cout) continue;
      tf_st4<VEC>(dW + (long long)orow * Cin, p, Cin, f32x4{acc[q][0][r], acc[q][1][r], acc[q][2][r], acc[q][3][r]});
    }
}

// ---------------------------------------------------------------------------------------------------------- attention

// probabilities of query `lane` into P[key][lane]; returns nothing else: the row is normalised in place
__device__ __forceinline__ void tf_attn_probs(const float* __restrict__ q, const float* __restrict__ k0, long long tok,
                                              int N, int hd, float scale, int lane, float* P) {
  float mx = -3.0e38f;
  for (int m = 0; m < N; ++m) {
    const float* __restrict__ km = k0 + m * tok;
    float dot = 0.f;
    for (int d = 0; d < hd; ++d) dot += q[d] * km[d];
    dot *= scale;
    P[m * kSStride + lane] = dot;
    mx = fmaxf(mx, dot);
  }
  float sum = 0.f;
  for (int m = 0; m < N; ++m) {
    const float e = expf(P[m * kSStride + lane] - mx);
    P[m * kSStride + lane] = e;
    sum += e;
  }
  const float inv = 1.0f / sum;
  for (int m = 0; m < N; ++m) P[m * kSStride + lane] *= inv;
}

// grid S * heads, 64 threads. qkv (S, N, 3, heads, hd), out (S, N, heads * hd)
__global__ __launch_bounds__(64) void tf_attn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N,
                                                         int heads, int hd, float scale) {
  __shared__ float P[kMaxN * kSStride];
  const int lane = threadIdx.x, h = blockIdx.x % heads;
  const long long s = blockIdx.x / heads, C = (long long)heads * hd, tok = 3 * C;
  const float* __restrict__ base = qkv + s * N * tok + (long long)h * hd;
  if (lane >= N) return;                                   // no barrier below: a lane reads only its own column of P
  tf_attn_probs(base + lane * tok, base + C, tok, N, hd, scale, lane, P);
  float* __restrict__ o = out + (s * N + lane) * C + (long long)h * hd;
  for (int d = 0; d < hd; ++d) {
    float a = 0.f;
    for (int m = 0; m < N; ++m) a += P[m * kSStride + lane] * base[2 * C + m * tok + d];
    o[d] = a;
  }
}

__global__ __launch_bounds__(64) void tf_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                         float* __restrict__ dqkv, int N, int heads, int hd,
                                                         float scale) {
  __shared__ float P[kMaxN * kSStride];
  __shared__ float dS[kMaxN * kSStride];
  const int lane = threadIdx.x, h = blockIdx.x % heads;
  const long long s = blockIdx.x / heads, C = (long long)heads * hd, tok = 3 * C;
  const float* __restrict__ base = qkv + s * N * tok + (long long)h * hd;
  const float* __restrict__ dbase = dout + s * N * C + (long long)h * hd;
  float* __restrict__ gbase = dqkv + s * N * tok + (long long)h * hd;
  const bool on = lane < N;
  if (on) {
    tf_attn_probs(base + lane * tok, base + C, tok, N, hd, scale, lane, P);
    const float* __restrict__ dn = dbase + lane * C;
    float D = 0.f;
    for (int m = 0; m < N; ++m) {                          // dP[n][m] = dout[n] . v[m]
      const float* __restrict__ vm = base + 2 * C + m * tok;
      float dp = 0.f;
      for (int d = 0; d < hd; ++d) dp += dn[d] * vm[d];
      dS[m * kSStride + lane] = dp;
      D += P[m * kSStride + lane] * dp;
    }
    for (int m = 0; m < N; ++m)
      dS[m * kSStride + lane] = P[m * kSStride + lane] * (dS[m * kSStride + lane] - D) * scale;
    float* __restrict__ dq = gbase + lane * tok;           // dq[n] = sum_m dS[n][m] k[m]
    for (int d = 0; d < hd; ++d) {
      float a = 0.f;
      for (int m = 0; m < N; ++m) a += dS[m * kSStride + lane] * base[C + m * tok + d];
      dq[d] = a;
    }
  }
  __syncthreads();
  if (!on) return;
  float* __restrict__ dk = gbase + C + lane * tok;         // lane = key m: rows of the tiles
  float* __restrict__ dv = gbase + 2 * C + lane * tok;
  for (int d = 0; d < hd; ++d) {
    float a = 0.f, b = 0.f;
    for (int n = 0; n < N; ++n) {
      a += dS[lane * kSStride + n] * base[n * tok + d];
      b += P[lane * kSStride + n] * dbase[n * C + d];
    }
    dk[d] = a;
    dv[d] = b;
  }
}

// --------------------------------------------------------------------------------------------- frame mean and add rows

__global__ __launch_bounds__(256) void tf_fmean_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ b, float* __restrict__ y,
                                                           long long S, int F, long long D) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= S * D) return;
  const long long s = i / D, d = i - s * D;
  float a = 0.f;
  for (int f = 0; f < F; ++f) a += w[f] * x[(s * F + f) * D + d];
  y[i] = b ? a + b[0] : a;
}

// blocks 0 .. F - 1: dw[f]; block F: db; blocks beyond: dx
__global__ __launch_bounds__(256) void tf_fmean_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ dy, float* __restrict__ dx,
                                                           float* __restrict__ dw, float* __restrict__ db, long long S,
                                                           int F, long long D) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x <= F) {
    // f64 sums: db is a sum of LayerNorm input gradients, whose rows cancel to zero - the partial sums of an f32
    // reduction are sqrt(S D) times larger than the result and their rounding is what would be left of it
    const int f = blockIdx.x;
    if (f < F ? dw == nullptr : db == nullptr) return;
    double a = 0.0;
    for (long long i = tid; i < S * D; i += 256) {
      const long long s = i / D, d = i - s * D;
      a += f < F ? (double)dy[i] * (double)x[(s * F + f) * D + d] : (double)dy[i];
    }
    red[tid] = a;
    __syncthreads();
    for (int n = 128; n > 0; n >>= 1) {
      if (tid < n) red[tid] += red[tid + n];
      __syncthreads();
    }
    if (tid == 0) (f < F ? dw[f] : db[0]) = (float)red[0];
    return;
  }
  if (!dx) return;
  const long long i = ((long long)blockIdx.x - F - 1) * 256 + tid;
  if (i >= S * F * D) return;
  const long long d = i % D, sf = i / D, s = sf / F;
  dx[i] = w[sf - s * F] * dy[s * D + d];
}

__global__ __launch_bounds__(256) void tf_add_rows_kernel(const float* __restrict__ x, const float* __restrict__ pos,
                                                          float* __restrict__ y, long long rows, int C, int period) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * C) return;
  const long long r = i / C;
  y[i] = x[i] + pos[(r % period) * C + (i - r * C)];
}

bool tf_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

int tf_rows_cols(const char* what, long long rows, int C, const char* cname) {
  HR_REQUIRE(rows >= 1 && rows <= kMaxRows, "%s: rows = %lld: needs 1 <= rows <= %lld", what, rows, kMaxRows);
  HR_REQUIRE(C >= 1 && C <= kMaxC, "%s: %s = %d: needs 1 <= %s <= %d", what, cname, C, cname, kMaxC);
  return HR_OK;
}

}  // namespace

extern "C" int hrnet_tf_supported(int op, int a, int b) {
  switch (op) {
    case HR_TF_LAYERNORM: return a >= 1 && a <= kMaxC;
    case HR_TF_LINEAR: return a >= 1 && a <= kMaxC && b >= 1 && b <= kMaxC;
    case HR_TF_ATTENTION: return a >= 1 && a <= kMaxN && b >= 1 && b <= kMaxHd;
    case HR_TF_FRAME_MEAN: return a >= 1 && a <= 65534;
    default: return 0;
  }
}

extern "C" long long hrnet_tf_layernorm_scratch(long long rows, int C) {
  if (rows < 1 || rows > kMaxRows || C < 1 || C > kMaxC) return 0;
  return 2 * rows + ((rows + kLnRows - 1) / kLnRows) * 2 * C;
}

extern "C" int hrnet_tf_layernorm(const float* x, const float* gamma, const float* beta, float* y, long long rows,
                                  int C, float eps, hr_stream_t stream) {
  if (const int rc = tf_rows_cols("tf_layernorm", rows, C, "C")) return rc;
  HR_REQUIRE(eps > 0.f, "tf_layernorm: eps = %g: must be positive", (double)eps);
  HR_REQUIRE(x && gamma && beta && y, "tf_layernorm: null pointer (x = %p, gamma = %p, beta = %p, y = %p)",
             (const void*)x, (const void*)gamma, (const void*)beta, (void*)y);
  HR_REQUIRE((const void*)x != (const void*)y, "tf_layernorm: y aliases x");
  tf_ln_fwd_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(x, gamma, beta, y, rows, C, eps);
  return hr_check_launch("tf_layernorm");
}

extern "C" int hrnet_tf_layernorm_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma,
                                      float* dbeta, float* scratch, long long scratch_floats, long long rows, int C,
                                      float eps, hr_stream_t stream) {
  if (const int rc = tf_rows_cols("tf_layernorm_bwd", rows, C, "C")) return rc;
  HR_REQUIRE(eps > 0.f, "tf_layernorm_bwd: eps = %g: must be positive", (double)eps);
  HR_REQUIRE(x && dy, "tf_layernorm_bwd: null pointer (x = %p, dy = %p)", (const void*)x, (const void*)dy);
  HR_REQUIRE(dx || dgamma || dbeta, "tf_layernorm_bwd: dx, dgamma and dbeta are all null: nothing to compute");
  HR_REQUIRE(!dx || gamma, "tf_layernorm_bwd: gamma is null with dx asked for");
  HR_REQUIRE(!dx || ((const void*)dx != (const void*)x && (const void*)dx != (const void*)dy),
             "tf_layernorm_bwd: dx aliases x or dy");
  const bool cols = dgamma || dbeta;
  if (cols) {
    HR_REQUIRE(scratch, "tf_layernorm_bwd: null scratch with dgamma / dbeta asked for");
    HR_REQUIRE(scratch_floats >= hrnet_tf_layernorm_scratch(rows, C), "tf_layernorm_bwd: scratch of %lld floats, "
               "%lld are needed (rows = %lld, C = %d)", scratch_floats, hrnet_tf_layernorm_scratch(rows, C), rows, C);
  }
  hipStream_t s = (hipStream_t)stream;
  tf_ln_dx_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, s>>>(x, gamma, dy, dx, cols ? scratch : nullptr, rows, C, eps);
  if (cols) {
    const int parts = (int)((rows + kLnRows - 1) / kLnRows);
    float* part = scratch + 2 * rows;
    tf_ln_cols_kernel<<<dim3((unsigned)((C + 63) / 64), (unsigned)parts), 64, 0, s>>>(x, dy, scratch, part, rows, C);
    tf_ln_cols_sum_kernel<<<(unsigned)((C + 63) / 64), 64, 0, s>>>(part, dgamma, dbeta, parts, C);
  }
  return hr_check_launch("tf_layernorm_bwd");
}

namespace {
int tf_linear_shape(const char* what, long long rows, int Cin, int Cout, int act) {
  if (const int rc = tf_rows_cols(what, rows, Cin, "Cin")) return rc;
  if (const int rc = tf_rows_cols(what, rows, Cout, "Cout")) return rc;
  HR_REQUIRE(act == HR_TF_ACT_NONE || act == HR_TF_ACT_GELU, "%s: act = %d: 0 (none) and 1 (exact GELU) are built", what,
             act);
  HR_REQUIRE((rows + 63) / 64 <= 65535, "%s: rows = %lld: too many for the grid", what, rows);
  return HR_OK;
}
}  // namespace

extern "C" int hrnet_tf_linear(const float* x, const float* W, const float* bias, const float* res,
                               const float* row_scale, float* y, float* pre, long long rows, int Cin, int Cout, int act,
                               hr_stream_t stream) {
  if (const int rc = tf_linear_shape("tf_linear", rows, Cin, Cout, act)) return rc;
  HR_REQUIRE(x && W && y, "tf_linear: null pointer (x = %p, W = %p, y = %p)", (const void*)x, (const void*)W, (void*)y);
  HR_REQUIRE((const void*)y != (const void*)x && (const void*)y != (const void*)W, "tf_linear: y aliases x or W");
  HR_REQUIRE(!pre || act == HR_TF_ACT_GELU, "tf_linear: pre given without an activation");
  HR_REQUIRE(!pre || ((const void*)pre != (const void*)y && (const void*)pre != (const void*)x),
             "tf_linear: pre aliases x or y");
  const bool vec = Cin % 4 == 0 && Cout % 4 == 0 && tf_aligned(x) && tf_aligned(W) && tf_aligned(y) &&
                   (!res || tf_aligned(res)) && (!pre || tf_aligned(pre));
  const dim3 grid((unsigned)((Cout + 15) / 16), (unsigned)((rows + 63) / 64));
  hipStream_t s = (hipStream_t)stream;
#define TF_GO(V, G) tf_linear_kernel<V, G><<<grid, 64 * kWaves, 0, s>>>(x, W, bias, res, row_scale, y, pre, rows, Cin, Cout)
  if (act == HR_TF_ACT_GELU) {
    if (vec) TF_GO(true, true); else TF_GO(false, true);
  } else {
    if (vec) TF_GO(true, false); else TF_GO(false, false);
  }
#undef TF_GO
  return hr_check_launch("tf_linear");
}

extern "C" int hrnet_tf_linear_bwd(const float* x, const float* W, const float* dy, const float* pre,
                                   const float* row_scale, float* dx, float* dW, float* db, long long rows, int Cin,
                                   int Cout, int act, hr_stream_t stream) {
  if (const int rc = tf_linear_shape("tf_linear_bwd", rows, Cin, Cout, act)) return rc;
  HR_REQUIRE(dy, "tf_linear_bwd: dy is null");
  HR_REQUIRE(dx || dW || db, "tf_linear_bwd: dx, dW and db are all null: nothing to compute");
  HR_REQUIRE(act == HR_TF_ACT_NONE || pre, "tf_linear_bwd: pre (the saved pre-activation) is null with act = GELU");
  HR_REQUIRE(!dx || W, "tf_linear_bwd: W is null with dx asked for");
  HR_REQUIRE(!dW || x, "tf_linear_bwd: x is null with dW asked for");
  HR_REQUIRE(!dx || ((const void*)dx != (const void*)dy && (const void*)dx != (const void*)x),
             "tf_linear_bwd: dx aliases dy or x");
  HR_REQUIRE(!dW || ((const void*)dW != (const void*)W && (const void*)dW != (const void*)dy),
             "tf_linear_bwd: dW aliases W or dy");
  const bool gelu = act == HR_TF_ACT_GELU;
  const bool vec0 = Cin % 4 == 0 && Cout % 4 == 0 && tf_aligned(dy) && (!gelu || tf_aligned(pre));
  hipStream_t s = (hipStream_t)stream;
  if (dx) {
    const bool vec = vec0 && tf_aligned(W) && tf_aligned(dx);
    const dim3 grid((unsigned)((Cin + 63) / 64), (unsigned)((rows + 63) / 64));
#define TF_GO(V, G) tf_linear_dx_kernel<V, G><<<grid, 64 * kWaves, 0, s>>>(dy, pre, row_scale, W, dx, rows, Cin, Cout)
    if (gelu) {
      if (vec) TF_GO(true, true); else TF_GO(false, true);
    } else {
      if (vec) TF_GO(true, false); else TF_GO(false, false);
    }
#undef TF_GO
  }
  if (dW || db) {
    const bool vec = vec0 && (!dW || (tf_aligned(x) && tf_aligned(dW)));
    const dim3 grid(dW ? (unsigned)((Cin + 63) / 64) : 1u, (unsigned)((Cout + 63) / 64));
#define TF_GO(V, G) tf_linear_dw_kernel<V, G><<<grid, 64, 0, s>>>(dy, pre, row_scale, x, dW, db, rows, Cin, Cout)
    if (gelu) {
      if (vec) TF_GO(true, true); else TF_GO(false, true);
    } else {
      if (vec) TF_GO(true, false); else TF_GO(false, false);
    }
#undef TF_GO
  }
  return hr_check_launch("tf_linear_bwd");
}

namespace {
int tf_attn_shape(const char* what, int S, int N, int heads, int hd) {
  HR_REQUIRE(hrnet_tf_supported(HR_TF_ATTENTION, N, hd), "%s: N = %d, hd = %d: needs 1 <= N <= %d tokens and "
             "1 <= hd <= %d", what, N, hd, kMaxN, kMaxHd);
  HR_REQUIRE(S >= 1 && heads >= 1, "%s: S = %d, heads = %d: both must be at least 1", what, S, heads);
  HR_REQUIRE((long long)S * heads <= 0x7fffffffLL && (long long)heads * hd <= kMaxC, "%s: S * heads = %lld workgroups "
             "or heads * hd = %lld columns: too many", what, (long long)S * heads, (long long)heads * hd);
  return HR_OK;
}
}  // namespace

extern "C" int hrnet_tf_attention(const float* qkv, float* out, int S, int N, int heads, int hd, float scale,
                                  hr_stream_t stream) {
  if (const int rc = tf_attn_shape("tf_attention", S, N, heads, hd)) return rc;
  HR_REQUIRE(qkv && out, "tf_attention: null pointer (qkv = %p, out = %p)", (const void*)qkv, (void*)out);
  HR_REQUIRE((const void*)qkv != (const void*)out, "tf_attention: out aliases qkv");
  tf_attn_fwd_kernel<<<(unsigned)(S * heads), 64, 0, (hipStream_t)stream>>>(qkv, out, N, heads, hd, scale);
  return hr_check_launch("tf_attention");
}

extern "C" int hrnet_tf_attention_bwd(const float* qkv, const float* dout, float* dqkv, int S, int N, int heads, int hd,
                                      float scale, hr_stream_t stream) {
  if (const int rc = tf_attn_shape("tf_attention_bwd", S, N, heads, hd)) return rc;
  HR_REQUIRE(qkv && dout && dqkv, "tf_attention_bwd: null pointer (qkv = %p, dout = %p, dqkv = %p)", (const void*)qkv,
             (const void*)dout, (void*)dqkv);
  HR_REQUIRE((const void*)dqkv != (const void*)qkv && (const void*)dqkv != (const void*)dout,
             "tf_attention_bwd: dqkv aliases qkv or dout");
  tf_attn_bwd_kernel<<<(unsigned)(S * heads), 64, 0, (hipStream_t)stream>>>(qkv, dout, dqkv, N, heads, hd, scale);
  return hr_check_launch("tf_attention_bwd");
}

namespace {
int tf_fmean_shape(const char* what, long long S, int F, long long D) {
  HR_REQUIRE(D >= 1 && D <= (1 << 24) && F >= 1 && F <= 65534, "%s: F = %d, D = %lld: needs 1 <= F <= 65534 and "
             "1 <= D <= 2^24", what, F, D);
  HR_REQUIRE(S >= 1 && S <= kMaxRows, "%s: S = %lld: needs 1 <= S <= %lld", what, S, kMaxRows);
  HR_REQUIRE(S * F <= (1LL << 31) / D, "%s: S * F * D = more than 2^31 elements (S = %lld, F = %d, D = %lld)", what, S, F,
             D);
  return HR_OK;
}
}  // namespace

extern "C" int hrnet_tf_frame_mean(const float* x, const float* w, const float* b, float* y, long long S, int F,
                                   long long D, hr_stream_t stream) {
  if (const int rc = tf_fmean_shape("tf_frame_mean", S, F, D)) return rc;
  HR_REQUIRE(x && w && y, "tf_frame_mean: null pointer (x = %p, w = %p, y = %p)", (const void*)x, (const void*)w,
             (void*)y);
  HR_REQUIRE((const void*)x != (const void*)y, "tf_frame_mean: y aliases x");
  tf_fmean_fwd_kernel<<<(unsigned)((S * D + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, w, b, y, S, F, D);
  return hr_check_launch("tf_frame_mean");
}

extern "C" int hrnet_tf_frame_mean_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db,
                                       long long S, int F, long long D, hr_stream_t stream) {
  if (const int rc = tf_fmean_shape("tf_frame_mean_bwd", S, F, D)) return rc;
  HR_REQUIRE(dy, "tf_frame_mean_bwd: dy is null");
  HR_REQUIRE(dx || dw || db, "tf_frame_mean_bwd: dx, dw and db are all null: nothing to compute");
  HR_REQUIRE(!dx || w, "tf_frame_mean_bwd: w is null with dx asked for");
  HR_REQUIRE(!dw || x, "tf_frame_mean_bwd: x is null with dw asked for");
  HR_REQUIRE(!dx || ((const void*)dx != (const void*)dy && (const void*)dx != (const void*)x),
             "tf_frame_mean_bwd: dx aliases dy or x");
  const long long blocks = F + 1 + (dx ? (S * F * D + 255) / 256 : 0);
  tf_fmean_bwd_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, w, dy, dx, dw, db, S, F, D);
  return hr_check_launch("tf_frame_mean_bwd");
}

extern "C" int hrnet_tf_add_rows(const float* x, const float* pos, float* y, long long rows, int C, int period,
                                 hr_stream_t stream) {
  if (const int rc = tf_rows_cols("tf_add_rows", rows, C, "C")) return rc;
  HR_REQUIRE(period >= 1 && rows % period == 0, "tf_add_rows: period = %d does not divide rows = %lld", period, rows);
  HR_REQUIRE(rows * C <= (1LL << 31) * 255, "tf_add_rows: rows * C = %lld elements: too many", rows * C);
  HR_REQUIRE(x && pos && y, "tf_add_rows: null pointer (x = %p, pos = %p, y = %p)", (const void*)x, (const void*)pos,
             (void*)y);
  tf_add_rows_kernel<<<(unsigned)((rows * C + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, pos, y, rows, C, period);
  return hr_check_launch("tf_add_rows");
}
