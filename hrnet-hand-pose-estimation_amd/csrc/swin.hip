// Swin kernels of swin_transformer, the reference's SwinPose (reference lib/models/swin_transformer.py): window attention
// with cyclic shift, zero padding, relative-position bias and the shift mask (:237-269, :317-368, :491-510), and the two
// space-to-depth gathers, patch merging fused with its LayerNorm (:390-415) and the rows of the patch embedding (:550-559).
// and their backward for training. Everything is f32, row-major, 64-bit element offsets; no float atomics: every sum has
// one fixed order, so a call is bit-reproducible. LayerNorm, the linear layers and GELU are transformer.hip's.
//
//   attention   one workgroup of 4 waves per (image, window, head). The window's tokens are found arithmetically from
//               token order - no partition, roll, pad or reverse pass: local token n = (r, c) of window (wy, wx) is
//               shifted-grid token (wy ws + r, wx ws + c), which is padded-grid token ((i + shift) mod Hp, (j + shift) mod
//               Wp); inside H x W it is a row of qkv, outside its q, k and v are the qkv bias (the reference pads after
//               norm1, before the qkv linear). q, k and v are staged in LDS in chunks of 32 head channels (one chunk for
//               hd <= 32, staged once), rows beyond ws * ws as zeros. S = q k^T (64 x 64) and O = P v run on
//               mfma_f32_16x16x4f32 (A: lane (i = l & 15, g = l >> 4) holds A[i][g], B: lane (j, g) holds B[g][j], D:
//               column = l & 15, row = 4 * (l >> 4) + register); wave w owns queries 16 w .. 16 w + 15. Logits and
//               probabilities stay in LDS ([query][key], stride 65); the softmax is 4 lanes per row, each over 16 keys in
//               a fixed order, combined by two shuffles. A key beyond ws * ws gets a probability of exactly 0.
//   merge_ln    one wave per output row: the four (row parity fastest) neighbours' channels, zeros beyond an odd H or W;
//               mean and centred second moment in f64 over the gathered row, as tf_row_stats.
//   patch_rows  one thread per element of the (B Hp Wp, Cin p p) matrix, column c p p + kh p + kw.
//   attention_bwd, merge_scatter, patch_rows_bwd, deconv_dgrad: described at their kernels below.
#include "common.h"

namespace {

constexpr int kTok = 64;               // tokens of a window, padded
constexpr int kMaxHd = 128;
constexpr int kChunk = 32;             // head channels staged at a time
constexpr int kQStride = kChunk + 4;   // LDS row stride of q / k / v: 16-byte reads of 16 rows fall on 16 distinct slots
constexpr int kSStride = kTok + 1;     // LDS row stride of the [query][key] tile
constexpr int kMaxC = 1 << 16;

#define SW_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

struct SwinAttn {
  const float* qkv;
  const float* qkv_bias;
  const float* table;
  float* out;
  int H, W, heads, hd, ws, shift, nwx, nwin;   // nwx: windows per row, nwin: windows per image
  float scale;
};

__device__ __forceinline__ int sw_band(int i, int Hp, int ws, int shift) { return i < Hp - ws ? 0 : (i < Hp - shift ? 1 : 2); }

// grid B * nwin * heads, 256 threads
__global__ __launch_bounds__(256) void swin_attn_kernel(const SwinAttn a) {
  __shared__ __attribute__((aligned(16))) float Qs[kTok * kQStride];
  __shared__ __attribute__((aligned(16))) float Ks[kTok * kQStride];
  __shared__ __attribute__((aligned(16))) float Vs[kTok * kQStride];
  __shared__ float P[kTok * kSStride];
  __shared__ int src[kTok];            // row of the image's tokens, -1: a token of the padded border, -2: beyond ws * ws
  __shared__ int reg[kTok];            // region id of the shift mask
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int h = blockIdx.x % a.heads;
  const int win = (blockIdx.x / a.heads) % a.nwin;
  const long long b = blockIdx.x / a.heads / a.nwin;
  const int ws = a.ws, N = ws * ws, hd = a.hd;
  const int Hp = (a.H + ws - 1) / ws * ws, Wp = (a.W + ws - 1) / ws * ws;
  const long long C = (long long)a.heads * hd, tok0 = b * a.H * a.W;
  if (tid < kTok) {
    int s = -2, r = 0;
    if (tid < N) {
      const int i = (win / a.nwx) * ws + tid / ws, jj = (win % a.nwx) * ws + tid % ws;
      const int pi = (i + a.shift) % Hp, pj = (jj + a.shift) % Wp;
      s = (pi < a.H && pj < a.W) ? pi * a.W + pj : -1;
      if (a.shift > 0) r = 3 * sw_band(i, Hp, ws, a.shift) + sw_band(jj, Wp, ws, a.shift);
    }
    src[tid] = s;
    reg[tid] = r;
  }
  __syncthreads();

  // rows [0, 64) x channels [d0, d0 + 32) of q (which = 0), k (1) or v (2) into LDS; zeros beyond N and hd
  auto stage = [&](float* dst, int which, int d0) {
    const float* __restrict__ bias = a.qkv_bias + which * C + (long long)h * hd;
    for (int idx = tid; idx < kTok * kChunk; idx += 256) {
      const int row = idx >> 5, d = d0 + (idx & 31);
      const int s = src[row];
      float v = 0.f;
      if (s != -2 && d < hd) v = s >= 0 ? a.qkv[(tok0 + s) * 3 * C + which * C + (long long)h * hd + d] : bias[d];
      dst[row * kQStride + (idx & 31)] = v;
    }
  };

  const int nchunk = (hd + kChunk - 1) / kChunk;
  f32x4 acc[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) acc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < nchunk; ++c) {
    if (c) __syncthreads();
    stage(Qs, 0, c * kChunk);
    stage(Ks, 1, c * kChunk);
    if (nchunk == 1) stage(Vs, 2, 0);
    __syncthreads();
    const int width = hd - c * kChunk < kChunk ? hd - c * kChunk : kChunk;
    for (int k0 = 0; k0 < width; k0 += 16) {               // A = q rows 16 wave + j, B = k rows 16 kt + j; k step e: channel 4 g + e
      const f32x4 qa = *(const f32x4*)(Qs + (16 * wave + j) * kQStride + k0 + 4 * g);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const f32x4 kb = *(const f32x4*)(Ks + (16 * kt + j) * kQStride + k0 + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[kt] = SW_MFMA(qa[e], kb[e], acc[kt]);
      }
    }
  }
  // D: lane (j, g) register r = query 16 wave + 4 g + r, key 16 kt + j
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    const int m = 16 * kt + j;
    const int rm = m / ws, cm = m % ws;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = 16 * wave + 4 * g + r;
      float v = 0.f;
      if (n < N && m < N) {
        const int rel = (n / ws - rm + ws - 1) * (2 * ws - 1) + (n % ws - cm + ws - 1);
        v = acc[kt][r] * a.scale + a.table[(long long)rel * a.heads + h];
        if (a.shift > 0 && reg[n] != reg[m]) v += -100.0f;
      }
      P[n * kSStride + m] = v;
    }
  }
  __syncthreads();
  {                                                        // softmax of row 16 wave + (lane >> 2), keys (lane & 3) + 4 t
    float* __restrict__ row = P + (16 * wave + (lane >> 2)) * kSStride;
    const int part = lane & 3;
    float mx = -3.0e38f;
    for (int m = part; m < N; m += 4) mx = fmaxf(mx, row[m]);
    mx = fmaxf(mx, __shfl_xor(mx, 1));
    mx = fmaxf(mx, __shfl_xor(mx, 2));
    float sum = 0.f;
    for (int m = part; m < N; m += 4) {
      const float e = expf(row[m] - mx);
      row[m] = e;
      sum += e;
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    for (int m = part; m < kTok; m += 4) row[m] = m < N ? row[m] / sum : 0.f;
  }
  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    if (nchunk > 1) {
      if (c) __syncthreads();
      stage(Vs, 2, c * kChunk);
      __syncthreads();
    }
    const int width = hd - c * kChunk < kChunk ? hd - c * kChunk : kChunk;
    for (int ct = 0; 16 * ct < width; ++ct) {              // A = P rows 16 wave + j, B = v; k step e: key 16 kc + 4 g + e
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        const int m0 = 16 * kc + 4 * g;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o = SW_MFMA(P[(16 * wave + j) * kSStride + m0 + e], Vs[(m0 + e) * kQStride + 16 * ct + j], o);
      }
      const int d = c * kChunk + 16 * ct + j;               // D: register r = query 16 wave + 4 g + r, column = channel d
      if (d < hd) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int s = src[16 * wave + 4 * g + r];
          if (s >= 0) a.out[(tok0 + s) * C + (long long)h * hd + d] = o[r];
        }
      }
    }
  }
}

struct SwinAttnBwd {
  const float* qkv;
  const float* qkv_bias;
  const float* table;
  const float* dout;
  float* dqkv;
  double* part;                                // one row of nbins + 2 hd f64 sums per workgroup, or null
  int H, W, heads, hd, ws, shift, nwx, nwin;
  float scale;
};

// grid B * nwin * heads, 256 threads: the forward's geometry. S and dP = dO v^T are accumulated together over the staged
// chunks; the [query][key] tile holds S, then P, then (after dV = P^T dO has read it) dS in place. dq = scale dS k and
// dk = scale dS^T q follow per chunk. A real token's dqkv row slice is written here and nowhere else; a padded key's dk and
// dv rows are summed in a fixed order (lane registers, two shuffles, waves 0 .. 3) into the workgroup's partial row, next
// to the (2 ws - 1)^2 bins of dS, one thread per bin. These sums of f32 products are kept in f64 from the first addition to
// the last, so dqkv_bias and dtable carry the rounding of their terms and one final rounding, not that of the partial sums.
__global__ __launch_bounds__(256) void swin_attn_bwd_kernel(const SwinAttnBwd a) {
  __shared__ __attribute__((aligned(16))) float Qs[kTok * kQStride];
  __shared__ __attribute__((aligned(16))) float Ks[kTok * kQStride];
  __shared__ __attribute__((aligned(16))) float Vs[kTok * kQStride];
  __shared__ __attribute__((aligned(16))) float Gs[kTok * kQStride];   // dO
  __shared__ float P[kTok * kSStride];
  __shared__ double wb[4 * 2 * kMaxHd];        // [wave][k, v][channel]: the padded keys' dk and dv sums of a wave
  __shared__ int src[kTok];
  __shared__ int reg[kTok];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int h = blockIdx.x % a.heads;
  const int win = (blockIdx.x / a.heads) % a.nwin;
  const long long b = blockIdx.x / a.heads / a.nwin;
  const int ws = a.ws, N = ws * ws, hd = a.hd;
  const int Hp = (a.H + ws - 1) / ws * ws, Wp = (a.W + ws - 1) / ws * ws;
  const long long C = (long long)a.heads * hd, tok0 = b * a.H * a.W;
  if (tid < kTok) {
    int s = -2, r = 0;
    if (tid < N) {
      const int i = (win / a.nwx) * ws + tid / ws, jj = (win % a.nwx) * ws + tid % ws;
      const int pi = (i + a.shift) % Hp, pj = (jj + a.shift) % Wp;
      s = (pi < a.H && pj < a.W) ? pi * a.W + pj : -1;
      if (a.shift > 0) r = 3 * sw_band(i, Hp, ws, a.shift) + sw_band(jj, Wp, ws, a.shift);
    }
    src[tid] = s;
    reg[tid] = r;
  }
  __syncthreads();

  // rows [0, 64) x channels [d0, d0 + 32) of q (which = 0), k (1), v (2) or dO (3) into LDS; zeros beyond N and hd, and
  // for the dO row of a padded token (its output row was dropped)
  auto stage = [&](float* dst, int which, int d0) {
    for (int idx = tid; idx < kTok * kChunk; idx += 256) {
      const int row = idx >> 5, d = d0 + (idx & 31);
      const int s = src[row];
      float v = 0.f;
      if (s != -2 && d < hd) {
        if (which == 3) v = s >= 0 ? a.dout[(tok0 + s) * C + (long long)h * hd + d] : 0.f;
        else v = s >= 0 ? a.qkv[(tok0 + s) * 3 * C + which * C + (long long)h * hd + d] : a.qkv_bias[which * C + (long long)h * hd + d];
      }
      dst[row * kQStride + (idx & 31)] = v;
    }
  };

  const int nchunk = (hd + kChunk - 1) / kChunk;
  f32x4 acc[4], dp[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) acc[kt] = dp[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < nchunk; ++c) {
    if (c) __syncthreads();
    stage(Qs, 0, c * kChunk);
    stage(Ks, 1, c * kChunk);
    stage(Vs, 2, c * kChunk);
    stage(Gs, 3, c * kChunk);
    __syncthreads();
    const int width = hd - c * kChunk < kChunk ? hd - c * kChunk : kChunk;
    for (int k0 = 0; k0 < width; k0 += 16) {               // A = q / dO rows 16 wave + j, B = k / v rows 16 kt + j
      const f32x4 qa = *(const f32x4*)(Qs + (16 * wave + j) * kQStride + k0 + 4 * g);
      const f32x4 ga = *(const f32x4*)(Gs + (16 * wave + j) * kQStride + k0 + 4 * g);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const f32x4 kb = *(const f32x4*)(Ks + (16 * kt + j) * kQStride + k0 + 4 * g);
        const f32x4 vb = *(const f32x4*)(Vs + (16 * kt + j) * kQStride + k0 + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[kt] = SW_MFMA(qa[e], kb[e], acc[kt]);
          dp[kt] = SW_MFMA(ga[e], vb[e], dp[kt]);
        }
      }
    }
  }
  // D: lane (j, g) register r = query 16 wave + 4 g + r, key 16 kt + j
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    const int m = 16 * kt + j;
    const int rm = m / ws, cm = m % ws;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = 16 * wave + 4 * g + r;
      float v = 0.f;
      if (n < N && m < N) {
        const int rel = (n / ws - rm + ws - 1) * (2 * ws - 1) + (n % ws - cm + ws - 1);
        v = acc[kt][r] * a.scale + a.table[(long long)rel * a.heads + h];
        if (a.shift > 0 && reg[n] != reg[m]) v += -100.0f;
      }
      P[n * kSStride + m] = v;
    }
  }
  __syncthreads();
  {                                                        // the forward's softmax, the same order
    float* __restrict__ row = P + (16 * wave + (lane >> 2)) * kSStride;
    const int part = lane & 3;
    float mx = -3.0e38f;
    for (int m = part; m < N; m += 4) mx = fmaxf(mx, row[m]);
    mx = fmaxf(mx, __shfl_xor(mx, 1));
    mx = fmaxf(mx, __shfl_xor(mx, 2));
    float sum = 0.f;
    for (int m = part; m < N; m += 4) {
      const float e = expf(row[m] - mx);
      row[m] = e;
      sum += e;
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    for (int m = part; m < kTok; m += 4) row[m] = m < N ? row[m] / sum : 0.f;
  }
  __syncthreads();

  // Y = T^T X for the staged chunk c: T the [query][key] tile, X rows = queries. Wave w owns keys 16 w .. 16 w + 15:
  // A lane (j, g) = T[query 16 kc + 4 g + e][key 16 wave + j], B lane (j, g) = X[that query][channel 16 ct + j];
  // D: register r = key 16 wave + 4 g + r, column = channel. Real keys go to third `which` of dqkv, padded keys to wb.
  auto keys_out = [&](const float* X, int c, int which, float mul) {
    const int width = hd - c * kChunk < kChunk ? hd - c * kChunk : kChunk;
    for (int ct = 0; 16 * ct < width; ++ct) {
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        const int n0 = 16 * kc + 4 * g;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o = SW_MFMA(P[(n0 + e) * kSStride + 16 * wave + j], X[(n0 + e) * kQStride + 16 * ct + j], o);
      }
      const int d = c * kChunk + 16 * ct + j;
      double pad = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = src[16 * wave + 4 * g + r];
        const float v = o[r] * mul;
        if (s >= 0) {
          if (d < hd) a.dqkv[(tok0 + s) * 3 * C + which * C + (long long)h * hd + d] = v;
        } else if (s == -1) {
          pad += (double)v;
        }
      }
      pad += __shfl_xor(pad, 16);
      pad += __shfl_xor(pad, 32);
      if (g == 0 && d < hd) wb[(wave * 2 + (which - 1)) * kMaxHd + d] = pad;
    }
  };

  for (int c = 0; c < nchunk; ++c) {                       // dV = P^T dO
    if (nchunk > 1) {
      if (c) __syncthreads();
      stage(Gs, 3, c * kChunk);
      __syncthreads();
    }
    keys_out(Gs, c, 2, 1.0f);
  }
  __syncthreads();
  {                                                        // dS = P (dP - rowsum(P dP)) in place, each lane its own D elements
    float delta[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) delta[r] += P[(16 * wave + 4 * g + r) * kSStride + 16 * kt + j] * dp[kt][r];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      delta[r] += __shfl_xor(delta[r], 1);
      delta[r] += __shfl_xor(delta[r], 2);
      delta[r] += __shfl_xor(delta[r], 4);
      delta[r] += __shfl_xor(delta[r], 8);
    }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float* __restrict__ p = P + (16 * wave + 4 * g + r) * kSStride + 16 * kt + j;
        *p = *p * (dp[kt][r] - delta[r]);
      }
  }
  __syncthreads();
  const int nb1 = 2 * ws - 1, nbins = nb1 * nb1;
  if (a.part && tid < nbins) {                             // bin (dr, dc): every (n, m) of the window with that offset
    const int dr = tid / nb1 - (ws - 1), dc = tid % nb1 - (ws - 1);
    double sum = 0.0;
    for (int rm = dr < 0 ? -dr : 0; rm < ws && rm + dr < ws; ++rm)
      for (int cm = dc < 0 ? -dc : 0; cm < ws && cm + dc < ws; ++cm)
        sum += (double)P[((rm + dr) * ws + cm + dc) * kSStride + rm * ws + cm];
    a.part[(long long)blockIdx.x * (nbins + 2 * hd) + tid] = sum;
  }
  for (int c = 0; c < nchunk; ++c) {
    if (nchunk > 1) {
      if (c) __syncthreads();
      stage(Qs, 0, c * kChunk);
      stage(Ks, 1, c * kChunk);
      __syncthreads();
    }
    const int width = hd - c * kChunk < kChunk ? hd - c * kChunk : kChunk;
    for (int ct = 0; 16 * ct < width; ++ct) {              // dq = scale dS k: the forward's P v with k in v's place
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        const int m0 = 16 * kc + 4 * g;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o = SW_MFMA(P[(16 * wave + j) * kSStride + m0 + e], Ks[(m0 + e) * kQStride + 16 * ct + j], o);
      }
      const int d = c * kChunk + 16 * ct + j;
      if (d < hd) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int s = src[16 * wave + 4 * g + r];
          if (s >= 0) a.dqkv[(tok0 + s) * 3 * C + (long long)h * hd + d] = o[r] * a.scale;
        }
      }
    }
    keys_out(Qs, c, 1, a.scale);                           // dk = scale dS^T q
  }
  if (a.part) {
    __syncthreads();
    if (tid < 2 * hd) {
      const int which = tid / hd, d = tid - which * hd;
      double sum = 0.0;
      for (int w = 0; w < 4; ++w) sum += wb[(w * 2 + which) * kMaxHd + d];
      a.part[(long long)blockIdx.x * (nbins + 2 * hd) + nbins + tid] = sum;
    }
  }
}

// grid ceil((nbins * heads + 3 C) / 256): one thread per output adds the workgroups' partial rows of its head in
// workgroup order, in f64. The q third of dqkv_bias is zero: a padded query's dS row is.
__global__ __launch_bounds__(256) void swin_attn_bwd_reduce_kernel(const double* __restrict__ part, float* __restrict__ dbias,
                                                                   float* __restrict__ dtable, long long per_head,
                                                                   int heads, int hd, int nbins) {
  const int C = heads * hd, rowlen = nbins + 2 * hd;
  const int i = blockIdx.x * 256 + threadIdx.x;
  int h, col;
  float* dst;
  if (i < nbins * heads) {
    if (!dtable) return;
    h = i % heads; col = i / heads; dst = dtable + i;
  } else {
    const int k = i - nbins * heads;
    if (k >= 3 * C || !dbias) return;
    dst = dbias + k;
    if (k < C) { *dst = 0.f; return; }
    const int which = k / C - 1, c = k % C;
    h = c / hd; col = nbins + which * hd + c % hd;
  }
  double s = 0.0;
  for (long long t = 0; t < per_head; ++t) s += part[(t * heads + h) * rowlen + col];
  *dst = (float)s;
}

__device__ __forceinline__ double sw_wave_sum64d(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// grid ceil(rows / 4), 256 threads: one wave per output row
__global__ __launch_bounds__(256) void swin_merge_ln_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ y,
                                                            long long rows, int H, int W, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int H2 = (H + 1) / 2, W2 = (W + 1) / 2, C4 = 4 * C;
  const int j2 = (int)(r % W2), i2 = (int)((r / W2) % H2);
  const long long b = r / W2 / H2;
  // block q of the row: pixel (2 i2 + (q & 1), 2 j2 + (q >> 1)); zeros beyond the map
  auto at = [&](int c) {
    const int q = c / C;
    const int i = 2 * i2 + (q & 1), j = 2 * j2 + (q >> 1);
    return (i < H && j < W) ? x[((b * H + i) * W + j) * C + (c - q * C)] : 0.f;
  };
  float* __restrict__ yr = y + r * C4;
  if (!gamma) {
    for (int c = lane; c < C4; c += 64) yr[c] = at(c);
    return;
  }
  double s = 0.0;
  for (int c = lane; c < C4; c += 64) s += (double)at(c);
  const double mean = sw_wave_sum64d(s) / (double)C4;
  double q2 = 0.0;
  for (int c = lane; c < C4; c += 64) {
    const double d = (double)at(c) - mean;
    q2 += d * d;
  }
  const double rstd = 1.0 / sqrt(sw_wave_sum64d(q2) / (double)C4 + (double)eps);
  for (int c = lane; c < C4; c += 64) yr[c] = (float)(((double)at(c) - mean) * rstd * (double)gamma[c] + (double)beta[c]);
}

// grid-stride over the elements of rows (B Hp Wp, Cin p p)
__global__ __launch_bounds__(256) void swin_patch_rows_kernel(const float* __restrict__ x, float* __restrict__ rows,
                                                              long long total, int Cin, int H, int W, int p) {
  const int Hp = (H + p - 1) / p, Wp = (W + p - 1) / p, K = Cin * p * p;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int col = (int)(i % K);
    const long long row = i / K;
    const int wp = (int)(row % Wp), hp = (int)((row / Wp) % Hp);
    const long long b = row / Wp / Hp;
    const int kw = col % p, kh = (col / p) % p, c = col / (p * p);
    const int yy = hp * p + kh, xx = wp * p + kw;
    rows[i] = (yy < H && xx < W) ? x[((b * Cin + c) * H + yy) * W + xx] : 0.f;
  }
}

// one thread per element of dx (B, H W, C): pixel (i, j) lies in row (i / 2, j / 2), block (i & 1) + 2 (j & 1)
__global__ __launch_bounds__(256) void swin_merge_scatter_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                                 long long total, int H, int W, int C) {
  const int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int c = (int)(t % C);
    const long long px = t / C;
    const int j = (int)(px % W), i = (int)((px / W) % H);
    const long long b = px / W / H;
    const int q = (i & 1) + 2 * (j & 1);
    dx[t] = dy[(((b * H2 + i / 2) * W2 + j / 2) * 4 + q) * C + c];
  }
}

// one thread per element of dx (B, Cin, H, W): pixel (y, x) is column c p p + (y % p) p + x % p of row (y / p, x / p)
__global__ __launch_bounds__(256) void swin_patch_rows_bwd_kernel(const float* __restrict__ drows, float* __restrict__ dx,
                                                                  long long total, int Cin, int H, int W, int p) {
  const int Hp = (H + p - 1) / p, Wp = (W + p - 1) / p;
  const long long K = (long long)Cin * p * p;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int xx = (int)(t % W), yy = (int)((t / W) % H), c = (int)((t / W / H) % Cin);
    const long long b = t / W / H / Cin;
    dx[t] = drows[((b * Hp + yy / p) * Wp + xx / p) * K + ((long long)c * p + yy % p) * p + xx % p];
  }
}

// Input gradient of ConvTranspose2d(Cin, Cout, 3, 2, 1, 1): dx[b, i, j, ci] = sum over taps (kh, kw) and co of
// du[b, 2 i - 1 + kh, 2 j - 1 + kw, co] * w[ci][tap][co] (taps outside the 2 H x 2 W map contribute nothing), w packed as
// the stride-2 convolution's forward weight [Cin_p][9][Cout_p]. grid (ceil(B H W / 64), ceil(Cin_p / 64)), 256 threads: a
// 64 pixel x 64 channel tile, the S = q k^T geometry of the attention kernel (A: pixels x 32 k, B: channels x 32 k in
// LDS). The sum has 9 Cout_p terms (3456 at 384 channels): each staged 32-term chunk runs in fresh f32 MFMA accumulators
// and is added to f64 totals, so the result carries the rounding of a 32-term chain, not of the whole sum.
__global__ __launch_bounds__(256) void swin_deconv_dgrad_kernel(const float* __restrict__ du, const float* __restrict__ w,
                                                                float* __restrict__ dx, long long M, int H, int W,
                                                                int Cop, int Cip) {
  __shared__ __attribute__((aligned(16))) float As[kTok * kQStride];
  __shared__ __attribute__((aligned(16))) float Bs[kTok * kQStride];
  __shared__ long long base[kTok];             // element offset of the pixel's (2 i - 1, 2 j - 1) corner, -1: no pixel
  __shared__ int pi[kTok], pj[kTok];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const long long p0 = (long long)blockIdx.x * kTok;
  const int c0 = blockIdx.y * kTok;
  if (tid < kTok) {
    const long long p = p0 + tid;
    int ii = -1, jj = -1;
    if (p < M) { jj = (int)(p % W); ii = (int)((p / W) % H); }
    pi[tid] = ii;
    pj[tid] = jj;
    base[tid] = p < M ? p / W / H : -1;        // the image
  }
  __syncthreads();
  double tot[4][4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) tot[kt][r] = 0.0;
  for (int tap = 0; tap < 9; ++tap) {
    const int kh = tap / 3, kw = tap % 3;
    for (int k0 = 0; k0 < Cop; k0 += kChunk) {
      __syncthreads();
      for (int idx = tid; idx < kTok * kChunk; idx += 256) {
        const int row = idx >> 5, k = k0 + (idx & 31);
        float a = 0.f, b = 0.f;
        const long long img = base[row];
        if (img >= 0 && k < Cop) {
          const int y = 2 * pi[row] - 1 + kh, x = 2 * pj[row] - 1 + kw;
          if (y >= 0 && y < 2 * H && x >= 0 && x < 2 * W) a = du[((img * 2 * H + y) * 2 * W + x) * Cop + k];
        }
        if (c0 + row < Cip && k < Cop) b = w[((long long)(c0 + row) * 9 + tap) * Cop + k];
        As[row * kQStride + (idx & 31)] = a;
        Bs[row * kQStride + (idx & 31)] = b;
      }
      __syncthreads();
      f32x4 acc[4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) acc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < kChunk; kk += 16) {
        const f32x4 av = *(const f32x4*)(As + (16 * wave + j) * kQStride + kk + 4 * g);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          const f32x4 bv = *(const f32x4*)(Bs + (16 * kt + j) * kQStride + kk + 4 * g);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[kt] = SW_MFMA(av[e], bv[e], acc[kt]);
        }
      }
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) tot[kt][r] += (double)acc[kt][r];
    }
  }
  // D: register r = pixel 16 wave + 4 g + r, column = channel c0 + 16 kt + j
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    const int c = c0 + 16 * kt + j;
    if (c >= Cip) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long p = p0 + 16 * wave + 4 * g + r;
      if (p < M) dx[p * Cip + c] = (float)tot[kt][r];
    }
  }
}

}  // namespace

extern "C" int hrnet_swin_supported(int op, int a, int b) {
  switch (op) {
    case HR_SWIN_ATTENTION: return a >= 1 && a <= 8 && b >= 1 && b <= kMaxHd;       // ws * ws <= 64
    case HR_SWIN_MERGE: return a >= 1 && a <= kMaxC / 4;
    case HR_SWIN_EMBED: return a >= 1 && b >= 1 && b <= 256 && (long long)a * b * b <= kMaxC;
    default: return 0;
  }
}

extern "C" int hrnet_swin_attention(const float* qkv, const float* qkv_bias, const float* bias_table, float* out, int B,
                                    int H, int W, int heads, int hd, int ws, int shift, float scale, hr_stream_t stream) {
  HR_REQUIRE(hrnet_swin_supported(HR_SWIN_ATTENTION, ws, hd), "swin_attention: ws = %d, hd = %d: needs 1 <= ws * ws <= %d "
             "tokens and 1 <= hd <= %d", ws, hd, kTok, kMaxHd);
  HR_REQUIRE(shift >= 0 && shift < ws, "swin_attention: shift = %d: needs 0 <= shift < ws = %d", shift, ws);
  HR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && heads >= 1, "swin_attention: B = %d, H = %d, W = %d, heads = %d: each must be at "
             "least 1", B, H, W, heads);
  HR_REQUIRE(H <= 16384 && W <= 16384 && (long long)heads * hd <= kMaxC, "swin_attention: H = %d, W = %d (at most 16384 "
             "each) or heads * hd = %lld columns (at most %d): too large", H, W, (long long)heads * hd, kMaxC);
  const int nwy = (H + ws - 1) / ws, nwx = (W + ws - 1) / ws;
  const long long groups = (long long)B * nwy * nwx * heads;
  HR_REQUIRE(groups <= 0x7fffffffLL, "swin_attention: %lld workgroups: too many", groups);
  HR_REQUIRE(qkv && qkv_bias && bias_table && out, "swin_attention: null pointer (qkv = %p, qkv_bias = %p, bias_table = %p, "
             "out = %p)", (const void*)qkv, (const void*)qkv_bias, (const void*)bias_table, (void*)out);
  HR_REQUIRE((const void*)qkv != (const void*)out, "swin_attention: out aliases qkv");
  SwinAttn a;
  a.qkv = qkv; a.qkv_bias = qkv_bias; a.table = bias_table; a.out = out;
  a.H = H; a.W = W; a.heads = heads; a.hd = hd; a.ws = ws; a.shift = shift; a.nwx = nwx; a.nwin = nwy * nwx;
  a.scale = scale;
  swin_attn_kernel<<<(unsigned)groups, 256, 0, (hipStream_t)stream>>>(a);
  return hr_check_launch("swin_attention");
}

extern "C" int hrnet_swin_merge_ln(const float* x, const float* gamma, const float* beta, float* y, int B, int H, int W,
                                   int C, float eps, hr_stream_t stream) {
  HR_REQUIRE(hrnet_swin_supported(HR_SWIN_MERGE, C, 0), "swin_merge_ln: C = %d: needs 1 <= 4 C <= %d", C, kMaxC);
  HR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "swin_merge_ln: B = %d, H = %d, W = %d: needs B >= 1 and "
             "1 <= H, W <= 16384", B, H, W);
  const long long rows = (long long)B * ((H + 1) / 2) * ((W + 1) / 2);
  HR_REQUIRE((rows + 3) / 4 <= 0x7fffffffLL, "swin_merge_ln: %lld rows: too many", rows);
  HR_REQUIRE((gamma == nullptr) == (beta == nullptr), "swin_merge_ln: gamma and beta come together (both null: the gather "
             "alone)");
  HR_REQUIRE(!gamma || eps > 0.f, "swin_merge_ln: eps = %g: must be positive", (double)eps);
  HR_REQUIRE(x && y, "swin_merge_ln: null pointer (x = %p, y = %p)", (const void*)x, (void*)y);
  HR_REQUIRE((const void*)x != (const void*)y, "swin_merge_ln: y aliases x");
  swin_merge_ln_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(x, gamma, beta, y, rows, H, W, C, eps);
  return hr_check_launch("swin_merge_ln");
}

extern "C" int hrnet_swin_patch_rows(const float* x, float* rows, int B, int Cin, int H, int W, int p,
                                     hr_stream_t stream) {
  HR_REQUIRE(hrnet_swin_supported(HR_SWIN_EMBED, Cin, p), "swin_patch_rows: Cin = %d, p = %d: needs 1 <= Cin * p * p <= %d",
             Cin, p, kMaxC);
  HR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "swin_patch_rows: B = %d, H = %d, W = %d: needs B >= 1 "
             "and 1 <= H, W <= 16384", B, H, W);
  const long long total = (long long)B * ((H + p - 1) / p) * ((W + p - 1) / p) * Cin * p * p;
  HR_REQUIRE(total <= (1LL << 40), "swin_patch_rows: %lld elements: too many", total);
  HR_REQUIRE(x && rows, "swin_patch_rows: null pointer (x = %p, rows = %p)", (const void*)x, (void*)rows);
  HR_REQUIRE((const void*)x != (const void*)rows, "swin_patch_rows: rows aliases x");
  const long long blocks = (total + 255) / 256;
  swin_patch_rows_kernel<<<(unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)), 256, 0, (hipStream_t)stream>>>(
      x, rows, total, Cin, H, W, p);
  return hr_check_launch("swin_patch_rows");
}

namespace {
int swin_attn_shape(const char* what, int B, int H, int W, int heads, int hd, int ws, int shift) {
  HR_REQUIRE(hrnet_swin_supported(HR_SWIN_ATTENTION, ws, hd), "%s: ws = %d, hd = %d: needs 1 <= ws * ws <= %d tokens and "
             "1 <= hd <= %d", what, ws, hd, kTok, kMaxHd);
  HR_REQUIRE(shift >= 0 && shift < ws, "%s: shift = %d: needs 0 <= shift < ws = %d", what, shift, ws);
  HR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && heads >= 1, "%s: B = %d, H = %d, W = %d, heads = %d: each must be at least 1",
             what, B, H, W, heads);
  HR_REQUIRE(H <= 16384 && W <= 16384 && (long long)heads * hd <= kMaxC, "%s: H = %d, W = %d (at most 16384 each) or "
             "heads * hd = %lld columns (at most %d): too large", what, H, W, (long long)heads * hd, kMaxC);
  const long long groups = (long long)B * ((H + ws - 1) / ws) * ((W + ws - 1) / ws) * heads;
  HR_REQUIRE(groups <= 0x7fffffffLL, "%s: %lld workgroups: too many", what, groups);
  return HR_OK;
}
}  // namespace

extern "C" int hrnet_swin_attention_bwd_scratch(int B, int H, int W, int heads, int hd, int ws) {
  if (!hrnet_swin_supported(HR_SWIN_ATTENTION, ws, hd) || B < 1 || H < 1 || W < 1 || heads < 1 || H > 16384 || W > 16384 ||
      (long long)heads * hd > kMaxC)
    return 0;
  const long long groups = (long long)B * ((H + ws - 1) / ws) * ((W + ws - 1) / ws) * heads;
  if (groups > 0x7fffffffLL) return 0;
  const long long floats = 2 * groups * ((2 * ws - 1) * (2 * ws - 1) + 2 * hd);     // f64 sums, two floats each
  return floats <= 0x7fffffffLL ? (int)floats : 0;
}

extern "C" int hrnet_swin_attention_bwd(const float* qkv, const float* qkv_bias, const float* bias_table,
                                        const float* dout, float* dqkv, float* dqkv_bias, float* dtable, float* scratch,
                                        long long scratch_floats, int B, int H, int W, int heads, int hd, int ws,
                                        int shift, float scale, hr_stream_t stream) {
  if (const int rc = swin_attn_shape("swin_attention_bwd", B, H, W, heads, hd, ws, shift)) return rc;
  HR_REQUIRE(qkv && qkv_bias && bias_table && dout && dqkv, "swin_attention_bwd: null pointer (qkv = %p, qkv_bias = %p, "
             "bias_table = %p, dout = %p, dqkv = %p)", (const void*)qkv, (const void*)qkv_bias, (const void*)bias_table,
             (const void*)dout, (void*)dqkv);
  HR_REQUIRE((const void*)dqkv != (const void*)qkv && (const void*)dqkv != (const void*)dout,
             "swin_attention_bwd: dqkv aliases qkv or dout");
  const bool sums = dqkv_bias || dtable;
  if (sums) {
    const long long need = hrnet_swin_attention_bwd_scratch(B, H, W, heads, hd, ws);
    HR_REQUIRE(need > 0, "swin_attention_bwd: the partial rows of dqkv_bias and dtable would take more than 2^31 floats: "
               "split the batch");
    HR_REQUIRE(scratch, "swin_attention_bwd: scratch is null (dqkv_bias and dtable are summed from it)");
    HR_REQUIRE(scratch_floats >= need, "swin_attention_bwd: scratch of %lld floats, %lld are needed", scratch_floats, need);
    HR_REQUIRE(((unsigned long long)scratch & 7ULL) == 0, "swin_attention_bwd: scratch %p is not 8-byte aligned (it holds "
               "f64 sums)", (void*)scratch);
    HR_REQUIRE((const void*)scratch != (const void*)qkv && (const void*)scratch != (const void*)dout &&
               (const void*)scratch != (const void*)dqkv && (const void*)scratch != (const void*)dqkv_bias &&
               (const void*)scratch != (const void*)dtable && (const void*)scratch != (const void*)qkv_bias &&
               (const void*)scratch != (const void*)bias_table, "swin_attention_bwd: scratch aliases another argument");
    HR_REQUIRE((const void*)dqkv_bias != (const void*)qkv_bias && (const void*)dtable != (const void*)bias_table &&
               (!dqkv_bias || (const void*)dqkv_bias != (const void*)dtable),
               "swin_attention_bwd: dqkv_bias or dtable aliases an input or each other");
  }
  const int nwy = (H + ws - 1) / ws, nwx = (W + ws - 1) / ws;
  const long long groups = (long long)B * nwy * nwx * heads;
  SwinAttnBwd a;
  a.qkv = qkv; a.qkv_bias = qkv_bias; a.table = bias_table; a.dout = dout; a.dqkv = dqkv; a.part = sums ? (double*)scratch : nullptr;
  a.H = H; a.W = W; a.heads = heads; a.hd = hd; a.ws = ws; a.shift = shift; a.nwx = nwx; a.nwin = nwy * nwx;
  a.scale = scale;
  hipStream_t s = (hipStream_t)stream;
  swin_attn_bwd_kernel<<<(unsigned)groups, 256, 0, s>>>(a);
  if (sums) {
    const int nbins = (2 * ws - 1) * (2 * ws - 1), outs = nbins * heads + 3 * heads * hd;
    swin_attn_bwd_reduce_kernel<<<(unsigned)((outs + 255) / 256), 256, 0, s>>>((const double*)scratch, dqkv_bias, dtable,
                                                                               (long long)B * nwy * nwx, heads, hd, nbins);
  }
  return hr_check_launch("swin_attention_bwd");
}

extern "C" int hrnet_swin_merge_scatter(const float* dy, float* dx, int B, int H, int W, int C, hr_stream_t stream) {
  HR_REQUIRE(hrnet_swin_supported(HR_SWIN_MERGE, C, 0), "swin_merge_scatter: C = %d: needs 1 <= 4 C <= %d", C, kMaxC);
  HR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "swin_merge_scatter: B = %d, H = %d, W = %d: needs "
             "B >= 1 and 1 <= H, W <= 16384", B, H, W);
  const long long total = (long long)B * H * W * C;
  HR_REQUIRE(total <= (1LL << 40), "swin_merge_scatter: %lld elements: too many", total);
  HR_REQUIRE(dy && dx, "swin_merge_scatter: null pointer (dy = %p, dx = %p)", (const void*)dy, (void*)dx);
  HR_REQUIRE((const void*)dy != (const void*)dx, "swin_merge_scatter: dx aliases dy");
  const long long blocks = (total + 255) / 256;
  swin_merge_scatter_kernel<<<(unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)), 256, 0, (hipStream_t)stream>>>(
      dy, dx, total, H, W, C);
  return hr_check_launch("swin_merge_scatter");
}

extern "C" int hrnet_swin_patch_rows_bwd(const float* drows, float* dx, int B, int Cin, int H, int W, int p,
                                         hr_stream_t stream) {
  HR_REQUIRE(hrnet_swin_supported(HR_SWIN_EMBED, Cin, p), "swin_patch_rows_bwd: Cin = %d, p = %d: needs 1 <= Cin * p * p "
             "<= %d", Cin, p, kMaxC);
  HR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "swin_patch_rows_bwd: B = %d, H = %d, W = %d: needs "
             "B >= 1 and 1 <= H, W <= 16384", B, H, W);
  const long long total = (long long)B * Cin * H * W;
  HR_REQUIRE(total <= (1LL << 40), "swin_patch_rows_bwd: %lld elements: too many", total);
  HR_REQUIRE(drows && dx, "swin_patch_rows_bwd: null pointer (drows = %p, dx = %p)", (const void*)drows, (void*)dx);
  HR_REQUIRE((const void*)drows != (const void*)dx, "swin_patch_rows_bwd: dx aliases drows");
  const long long blocks = (total + 255) / 256;
  swin_patch_rows_bwd_kernel<<<(unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)), 256, 0, (hipStream_t)stream>>>(
      drows, dx, total, Cin, H, W, p);
  return hr_check_launch("swin_patch_rows_bwd");
}

extern "C" int hrnet_swin_deconv_dgrad(const float* du, const float* w_packed, float* dx, int B, int H, int W, int Cout_p,
                                       int Cin_p, hr_stream_t stream) {
  HR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192, "swin_deconv_dgrad: B = %d, H = %d, W = %d: needs B >= 1 "
             "and 1 <= H, W <= 8192", B, H, W);
  HR_REQUIRE(Cout_p >= 4 && Cout_p % 4 == 0 && Cin_p >= 4 && Cin_p % 4 == 0 && Cout_p <= kMaxC && Cin_p <= kMaxC,
             "swin_deconv_dgrad: Cout_p = %d, Cin_p = %d: multiples of 4, at most %d", Cout_p, Cin_p, kMaxC);
  const long long M = (long long)B * H * W;
  HR_REQUIRE((M + kTok - 1) / kTok <= 0x7fffffffLL, "swin_deconv_dgrad: %lld pixels: too many", M);
  HR_REQUIRE(du && w_packed && dx, "swin_deconv_dgrad: null pointer (du = %p, w_packed = %p, dx = %p)", (const void*)du,
             (const void*)w_packed, (void*)dx);
  HR_REQUIRE((const void*)dx != (const void*)du && (const void*)dx != (const void*)w_packed,
             "swin_deconv_dgrad: dx aliases an input");
  const dim3 grid((unsigned)((M + kTok - 1) / kTok), (unsigned)((Cin_p + kTok - 1) / kTok));
  swin_deconv_dgrad_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(du, w_packed, dx, M, H, W, Cout_p, Cin_p);
  return hr_check_launch("swin_deconv_dgrad");
}
